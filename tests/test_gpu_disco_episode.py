"""Closed-loop MultiDISCO episodes on the device (csrc/disco_batch.hpp disco_episode_kernel / disco_skid_nav_episode_kernel,
dust_disco_batch_episode, `DiscoBatch.episode`, `BatchDISCO.run_episodes` / `simulate`): T periods of forward, step, plant step and
records in ONE launch, optionally under the reference's episode rules.  Every np.array_equal below is bit for bit.

1. an episode is its periods: episode(T) under rules against T ticks of a clone fed the episode's own recorded states, the host applying
   the rules through the fp32 replicas of tests/svmpc_sim_cases.py and deactivating stopped environments - actions, status, n_run, every
   getter, the last a_seq, one further tick on both; the forced events of tests/disco_cases.py happen where they were proved; rows past
   n_run are unwritten; loss is the sequential fp32 sum of the cost rows, and inf exactly after a crash;
2. the plant: every recorded state against the float64 step on the device's OWN previous state and action within the plant tolerance of
   tests/svmpc_episode_cases.py, and at least 5 tolerances from its wrong plants; every cost against the float64 cost of that state;
3. rules NULL against rules that never fire; DUST_DISCO_PARAMS_ONCE against the replicated [T] array;
4. two chained calls against one, split before and after a stop;
5. an environment does not depend on its batch;
6. one launch per call, every refusal with zero launches and unchanged getters and in-out arrays;
7. `BatchDISCO.run_episodes` / `simulate` against tick() of the class, a deep copy mid-loop; both drivers against `simulate` called
   directly; the example's --tiny.
"""
import copy
import functools
import importlib.util
import os

import numpy as np
import pytest
import torch

import disco_cases as dc
import svmpc_episode_cases as ec
import svmpc_sim_cases as sc
from helpers import elemerr
from disco_helpers import GETTERS, _L, _batch, _grid, _pair, _records, _same, _sub

pytestmark = pytest.mark.gpu


def _rules(case, on=True, t0=0):
    r = dc.RULES[case["id"]]
    if not on:
        return dict(t0=t0)
    return dict(t0=t0, goal=r["goal"], goal_radius=r["radius"], stop_on_crash=r["crash"])


def _cell(case):
    return dc.ac.PART["cell"] if case["family"] == "particle" else dc.NAV["cell_size"]


def _host_status(case, x):
    """status [n] of fp32 states x by the fp32 replicas: 2 crash (wins), 1 goal, 0 neither"""
    r = dc.RULES[case["id"]]
    st = np.zeros(len(x), np.int32)
    if r["goal"] is not None:
        st[sc.goal32(r["goal"], r["radius"], x)] = 1
    if r["crash"]:
        st[sc.crashed32(_grid(case), x[:, :2], _cell(case))] = 2
    return st


def _episode_inputs(case, T):
    inp = dc.inputs(case)
    inp["plant"] = dc.plant_rows(case)
    inp["eparams"] = dc.episode_params(case, T + 1)  # (one more period: the further tick)
    return inp


@functools.lru_cache(maxsize=None)
def _run(cid):
    """the case's episode under its rules and, on a clone taken before it, its periods as ticks fed the recorded states"""
    case = dc.BY_ID[cid]
    T, B, strat = case["T"], case["B"], case["strategy"]
    inp = _episode_inputs(case, T)
    b = _batch(case, inp)
    twin = b.clone()
    ep = None if inp["eparams"] is None else inp["eparams"][:T]
    xs, acts, costs, loss, status, n_run, a_seq = b.episode(inp["states"], T, strat, ep, inp["plant"], rules=_rules(case))
    x, on, ticks, hstat, hrun = inp["states"].copy(), np.ones(B, bool), [], np.zeros(B, np.int32), np.zeros(B, np.int32)
    for t in range(T):
        if not on.any():
            break
        ticks.append((on.copy(), twin.tick(x, strat, 1, params=None if ep is None else ep[t], active=on)))
        x = np.where(on[:, None], xs[t], x)
        st = _host_status(case, x)
        hrun[on] += 1
        hstat[on] = st[on]
        on = on & (st == 0)
    out = dict(inp=inp, xs=xs, acts=acts, costs=costs, loss=loss, status=status, n_run=n_run, a_seq=a_seq, ticks=ticks, hstat=hstat, hrun=hrun,
               after=(_records(b), _records(twin)), still=on.copy())
    extra = None if inp["eparams"] is None else inp["eparams"][T]
    if on.any():
        out["further"] = (b.tick(x, strat, 1, params=extra, active=on), twin.tick(x, strat, 1, params=extra, active=on), _records(b), _records(twin))
    b.close()
    twin.close()
    return out


# ------------------------------------------------------------------------------------------------ 1. an episode is its periods
@pytest.mark.parametrize("cid", dc.EPISODE_IDS)
def test_episode_equals_its_periods(cid):
    case, r = dc.BY_ID[cid], _run(cid)
    T, B, f = case["T"], case["B"], dc.family(case)
    assert r["xs"].shape == (T, B, f["ds"]) and r["acts"].shape == (T, B, f["da"]) and r["costs"].shape == (T, B)
    assert np.array_equal(r["status"], r["hstat"]) and np.array_equal(r["n_run"], r["hrun"]), (r["status"], r["hstat"], r["n_run"], r["hrun"])
    for e, (period, status) in dc.EVENTS.get(cid, {}).items():
        assert r["n_run"][e] == period + 1 and r["status"][e] == status, (e, r["n_run"][e], r["status"][e])
    for e in range(B):
        n = int(r["n_run"][e])
        assert np.isfinite(r["xs"][:n, e]).all() and np.isfinite(r["acts"][:n, e]).all() and np.isfinite(r["costs"][:n, e]).all()
        assert np.isnan(r["xs"][n:, e]).all() and np.isnan(r["acts"][n:, e]).all() and np.isnan(r["costs"][n:, e]).all()  # rows past n_run
        acc = np.float32(0.0)
        for t in range(n):
            acc = np.float32(acc + r["costs"][t, e])
        if r["status"][e] == 2:
            assert np.isposinf(r["loss"][e]), e
        else:
            assert np.float32(r["loss"][e]) == acc and np.isfinite(r["loss"][e]), (e, r["loss"][e], acc)
    for t, (on, nxt) in enumerate(r["ticks"]):
        assert np.array_equal(nxt[on, 0], r["acts"][t][on]), t
    _same(*r["after"])
    assert np.array_equal(r["a_seq"], r["after"][0]["A_SEQ"])
    if "further" in r:
        n1, n2, g1, g2 = r["further"]
        assert np.array_equal(n1[r["still"]], n2[r["still"]])
        _same(g1, g2)
    if T > 1 and (r["n_run"] > 1).any() and case["H"] > 1:  # (the periods are not copies of one another)
        e = int(np.argmax(r["n_run"] > 1))
        assert not np.array_equal(r["acts"][0, e], r["acts"][1, e])


# ------------------------------------------------------------------------------------------------ 2. the plant and the cost
@pytest.mark.parametrize("cid", dc.EPISODE_IDS)
def test_plant_steps_and_costs_against_float64(cid):
    """stage-wise: states_out[t] against the float64 step of (states_{t-1}, actions_out[t], the true row), costs_out[t] against the
    float64 cost of states_out[t] - the device's own previous state and action, never a whole trajectory"""
    case, r = dc.BY_ID[cid], _run(cid)
    grid = _grid(case)
    pgrid = grid if case["family"] == "particle" else None
    rows, B = r["inp"]["plant"], case["B"]
    # the plant tolerance of tests/svmpc_episode_cases.py for this family's plant (its cases carry the family's constants; `one` is the
    # Pendulum's): measured there from the float64 step alone
    fam = {"pendulum": "pend", "particle": "part", "skid": "skid", "cartpole": "cart"}[case["family"]]
    tol = ec.plant_tolerance(ec.BY_ID[fam], pgrid)
    # (... and the cost tolerance of tests/svmpc_sim_cases.py; its skid-steer case is the navigation one: the plain cost is its first term)
    ctol = sc.cost_tolerance(sc.BY_ID["skid_nav" if case["family"] == "skid" else fam])
    got, ref, cgot, cref, var = [], [], [], [], {}
    for e in range(B):
        n = int(r["n_run"][e])
        prev = np.concatenate((r["inp"]["states"][e][None], r["xs"][:n - 1, e]))
        row = None if rows is None else np.repeat(rows[e][None], n, 0)
        got.append(r["xs"][:n, e])
        ref.append(ec.plant_step(case, prev, r["acts"][:n, e], row, pgrid))
        for t in range(n):
            for k, v in ec.variant_steps(case, prev[t:t + 1], r["acts"][t:t + 1, e], r["acts"][t - 1:t, e] if t else None,
                                         None if rows is None else rows[e][None], pgrid).items():
                var.setdefault(k, []).append((len(np.concatenate(got)) - n + t, v[0]))
        cgot.append(r["costs"][:n, e])
        c = dc.ac._costs(case, r["xs"][:n, e].astype(np.float64), grid, False)
        if case["nav"]:
            c = c + dc.NAV["w_obs"] * dc.ac._collisions(grid, r["xs"][:n, e, :2].astype(np.float64), dc.NAV["cell_size"])
        cref.append(c)
    got, ref, cgot, cref = (np.concatenate(v) for v in (got, ref, cgot, cref))
    err, cerr = elemerr(got, ref), elemerr(cgot, cref)
    far = {}
    for k, v in var.items():
        idx = [i for i, _ in v]
        far[k] = elemerr(got[idx], np.stack([x for _, x in v])) / tol
    print("%-15s plant err %.2e tol %.2e  cost err %.2e tol %.2e  " % (cid, err, tol, cerr, ctol) + "  ".join("%s %.0f" % kv for kv in sorted(far.items())))
    assert err < tol, (cid, err, tol)
    assert cerr < ctol, (cid, cerr, ctol)
    for k, v in far.items():
        assert v >= 5.0, (cid, k, v)
    assert "unstepped" in far and (rows is None or "nominal" in far)


# ------------------------------------------------------------------------------------------------ 3. rules off, parameters once
@pytest.mark.parametrize("cid", ["mppi", "disco", "skid", "cart"])
def test_no_rules_is_rules_that_never_fire_and_params_once(cid):
    case, r = dc.BY_ID[cid], _run(cid)
    T, strat, inp = case["T"], case["strategy"], r["inp"]
    assert (r["n_run"] == T).all() and not r["status"].any()  # (the case's goal is out of reach)
    ep = None if inp["eparams"] is None else inp["eparams"][:T]
    b = _batch(case, inp)
    xs, acts, a_seq = b.episode(inp["states"], T, strat, ep, inp["plant"])
    got = _records(b)
    b.close()
    assert np.array_equal(xs, r["xs"]) and np.array_equal(acts, r["acts"]) and np.array_equal(a_seq, r["a_seq"])
    _same(got, r["after"][0])
    if ep is None:
        return
    once = np.ascontiguousarray(ep[0])
    b1, bT = _batch(case, inp), _batch(case, inp)
    o1 = b1.episode(inp["states"], T, strat, once, inp["plant"], params_once=True)
    oT = bT.episode(inp["states"], T, strat, np.ascontiguousarray(np.broadcast_to(once, ep.shape)), inp["plant"])
    for u, v in zip(o1, oT):
        assert np.array_equal(u, v)
    _same(_records(b1), _records(bT))
    assert not np.array_equal(o1[0], xs)  # (the periods' own rows differ from period 0's)
    b1.close()
    bT.close()


# ------------------------------------------------------------------------------------------------ 4. chaining
@pytest.mark.parametrize("cid,T1", [("part", 1), ("part", 2), ("mppi", 2), ("skid_nav_sigma", 1)])
def test_two_chained_calls_are_one(cid, T1):
    """`part`: environments 0 and 1 stop in period 0, environment 2 in period 1 - T1 = 1 splits after the first stops and before the
    last, T1 = 2 after all of them"""
    case, r = dc.BY_ID[cid], _run(cid)
    T, strat, inp = case["T"], case["strategy"], r["inp"]
    ep = None if inp["eparams"] is None else inp["eparams"][:T]
    b = _batch(case, inp)
    x1, a1, c1, loss, status, n1, _ = b.episode(inp["states"], T1, strat, None if ep is None else ep[:T1], inp["plant"], rules=_rules(case))
    x = np.where((n1 > 0)[:, None], x1[np.maximum(n1, 1) - 1, np.arange(case["B"])], inp["states"])
    x2, a2, c2, loss, status, n2, s2 = b.episode(x, T - T1, strat, None if ep is None else ep[T1:], inp["plant"], rules=_rules(case, t0=T1),
                                                 loss=loss, status=status)
    got = _records(b)
    b.close()
    assert np.array_equal(n1 + n2, r["n_run"]) and np.array_equal(status, r["status"])
    assert np.array_equal(loss, r["loss"])  # (inf == inf)
    for u, v, w in ((x1, x2, r["xs"]), (a1, a2, r["acts"]), (c1, c2, r["costs"])):
        both = np.concatenate((u, v))
        assert np.array_equal(np.nan_to_num(both, nan=7.0), np.nan_to_num(w, nan=7.0))
    stopped_early = n2 == 0
    assert np.isnan(s2[stopped_early]).all() and np.array_equal(s2[~stopped_early], r["a_seq"][~stopped_early])
    _same(got, r["after"][0])


# ------------------------------------------------------------------------------------------------ 5. independence from the batch
@pytest.mark.parametrize("cid", ["disco", "part", "skid_nav_sigma"])
def test_an_environment_does_not_depend_on_its_batch(cid):
    case, r = dc.BY_ID[cid], _run(cid)
    T, strat, inp, e, B = case["T"], case["strategy"], r["inp"], 1, case["B"]

    def episode(b, envs, active=None):
        ep = None if inp["eparams"] is None else np.ascontiguousarray(inp["eparams"][:T][:, list(envs)])
        return b.episode(_sub(inp, envs, "states"), T, strat, ep, _sub(inp, envs, "plant"), rules=_rules(case), active=active)

    want = [r[k][:, e] for k in ("xs", "acts", "costs")] + [r[k][e] for k in ("loss", "status", "n_run", "a_seq")]
    ref = {k: v[e] for k, v in r["after"][0].items()}
    eq = lambda u, v: np.array_equal(np.nan_to_num(u, nan=7.0), np.nan_to_num(v, nan=7.0))

    def check(out, got, slot):
        for k in range(3):
            assert eq(out[k][:, slot], want[k]), (k, slot)
        for k in range(3, 7):
            assert eq(out[k][slot], want[k]), (k, slot)
        for k in GETTERS:
            assert np.array_equal(got[k][slot], ref[k]), (k, slot)

    alone = _batch(case, inp, [e])
    check(episode(alone, [e]), _records(alone), 0)
    alone.close()
    envs = [e, 0, e, (e + 1) % B, e]  # slots 0 / 2 / 4 of five: beside neighbours that stop earlier, later or never
    five = _batch(case, inp, envs)
    out, got = episode(five, envs), _records(five)
    five.close()
    for slot in (0, 2, 4):
        check(out, got, slot)
    envs = [0, e, 0]  # beside inactive neighbours: a tick first, so that they have getters to keep
    three = _batch(case, inp, envs)
    three.tick(_sub(inp, envs, "states"), strat, 1, params=_sub(inp, envs, "params"))
    lone = _batch(case, inp, [e])
    lone.tick(_sub(inp, [e], "states"), strat, 1, params=_sub(inp, [e], "params"))
    before = _records(three)
    out, got = episode(three, envs, active=[0, 1, 0]), _records(three)
    solo, solo_got = episode(lone, [e]), _records(lone)
    three.close()
    lone.close()
    for k in range(3):  # [T, 3, .] records; the neighbours' rows are never written: NaN on the host
        assert eq(out[k][:, 1], solo[k][:, 0]) and np.isnan(out[k][:, [0, 2]]).all(), k
    assert eq(out[6][1], solo[6][0]) and np.isnan(out[6][[0, 2]]).all()
    assert out[5][1] == solo[5][0] and (out[5][[0, 2]] == -1).all()  # n_run
    for k in GETTERS:
        assert np.array_equal(got[k][1], solo_got[k][0]), k
        assert np.array_equal(got[k][[0, 2]], before[k][[0, 2]]), k


# ------------------------------------------------------------------------------------------------ 6. plumbing
def test_one_launch_per_episode_and_refusals_before_any_launch():
    L = _L()
    case = dc.BY_ID["multi_arg"]
    T, B, H = 3, case["B"], case["H"]
    inp = _episode_inputs(case, T)
    b = _batch(case, inp)
    b.ctx.profile(True)
    total = lambda: sum(v[1] for v in b.ctx.profile_get().values())
    ep = inp["eparams"][:T]
    b.episode(inp["states"], 1, "argmax", ep[:1], inp["plant"])
    assert total() == 1
    b.episode(inp["states"], T, "average", ep, inp["plant"], rules=dict(goal=(0.0, 0.0), goal_radius=0.5))
    assert total() == 2
    before = _records(b)
    lib, FP, IP = L.load(), L.FP, __import__("ctypes").POINTER(__import__("ctypes").c_int)
    keep = [np.ascontiguousarray(a, np.float32) for a in (inp["states"], ep, inp["plant"])]
    sp, pp, lp = (a.ctypes.data_as(FP) for a in keep)
    xs, ac, co, sq, loss = (np.zeros(s, np.float32) for s in ((T, B, 2), (T, B, 1), (T, B), (B, H, 1), (B,)))
    status, n_run = np.zeros(B, np.int32), np.full(B, -1, np.int32)
    ru = L.EpisodeRules()
    ru.goal_radius = 0.0
    import ctypes as C

    def call(states=sp, T_=T, prm=pp, plt=lp, strat=0, rules=ru, flags=0, so=xs, ao=ac, cost=co, ls=loss, stt=status, nr=n_run):
        P = lambda a: None if a is None else a.ctypes.data_as(FP)
        I = lambda a: None if a is None else a.ctypes.data_as(IP)
        return lib.dust_disco_batch_episode(b._h, states, T_, prm, plt, strat, None if rules is None else C.byref(rules), flags, None, P(so), P(ao),
                                            P(cost), P(ls), I(stt), I(nr), P(sq))

    warm, neg, crash = L.EpisodeRules(), L.EpisodeRules(), L.EpisodeRules()
    warm.warm_up, neg.t0, crash.stop_on_crash = 1, -1, 1
    nan_goal = L.EpisodeRules()
    nan_goal.goal_radius = float("nan")
    bad_status = np.array([0, 3, 0], np.int32)[:B]
    big = np.zeros((4097, B, case["M"], 1), np.float32).ctypes.data_as(FP)
    refused = [(call(states=None), L.ERR_INVALID), (call(so=None), L.ERR_INVALID), (call(ao=None), L.ERR_INVALID), (call(T_=0), L.ERR_INVALID),
               (call(T_=4097, prm=big), L.ERR_INVALID), (call(prm=None), L.ERR_INVALID), (call(strat=L.STEP_EXTERNAL), L.ERR_INVALID),
               (call(strat=3), L.ERR_INVALID), (call(rules=warm), L.ERR_INVALID), (call(rules=neg), L.ERR_INVALID), (call(rules=nan_goal), L.ERR_INVALID),
               (call(cost=None), L.ERR_INVALID), (call(ls=None), L.ERR_INVALID), (call(stt=None), L.ERR_INVALID), (call(nr=None), L.ERR_INVALID),
               (call(stt=bad_status), L.ERR_INVALID), (call(rules=crash), L.ERR_UNSUPPORTED), (call(flags=L.SVMPC_BATCH_KEEP_ACTIONS), L.ERR_UNSUPPORTED),
               (call(flags=L.PTR_DEVICE), L.ERR_UNSUPPORTED), (call(flags=L.EPS_AROUND_A_MAT), L.ERR_UNSUPPORTED)]
    for k, (got, want) in enumerate(refused):
        assert got == want, (k, got, want)
    assert total() == 2
    _same(_records(b), before)
    assert not xs.any() and not ac.any() and not co.any() and not sq.any() and not loss.any() and not status.any() and (n_run == -1).all()
    assert call(rules=None, cost=None, ls=None, stt=None, nr=None) == L.OK and total() == 3  # rules NULL: no cost / loss / status / n_run
    b.close()
    c0 = dc.BY_ID["mppi"]  # dim_p = 0: neither parameter rows nor true rows
    i0 = _episode_inputs(c0, 1)
    b0 = _batch(c0, i0)
    b0.ctx.profile(True)
    row = np.ones((1, c0["B"], 1, 1), np.float32)
    for kw in (dict(params=row), dict(plant_params=row.reshape(c0["B"], 1))):
        with pytest.raises(L.DustError) as e:
            b0.episode(i0["states"], 1, "average", **kw)
        assert e.value.status == L.ERR_INVALID
    assert sum(v[1] for v in b0.ctx.profile_get().values()) == 0
    b0.close()


# ------------------------------------------------------------------------------------------------ 7. the class
def test_run_episodes_and_simulate_against_ticks_of_the_class():
    """run_episodes(T) draws its dynamics rows as T ticks do: under one torch seed, T calls of tick() on a deep copy, fed the recorded
    states, give the same actions bit for bit; simulate() under rules that never fire is run_episodes(); a deep copy between two episodes
    continues identically"""
    import torch.distributions as dist

    B, T, seeds = 3, 3, [31, 32, 33]
    model, ep, _ = _pair(B, seeds)
    pd = dist.Independent(dist.Uniform(torch.tensor([0.8, 0.8]), torch.tensor([1.2, 1.2])), 1)
    true = torch.tensor([[1.2, 0.8], [0.8, 1.1], [1.0, 1.3]])
    st0 = torch.tensor([[3.0, 0.0], [2.5, 0.2], [3.4, -0.1]])
    torch.manual_seed(39)
    ep.tick(st0, model, pd, "average", 1)  # (creates the device batch, so that the deep copies below carry one)
    ticks, sim = copy.deepcopy(ep), copy.deepcopy(ep)
    torch.manual_seed(40)
    xs, acts, a_seq = ep.run_episodes(st0, model, pd, T, "average", plant_params=true)
    after = torch.rand(1)
    assert tuple(xs.shape) == (T, B, 2) and tuple(acts.shape) == (T, B, 1) and tuple(a_seq.shape) == (B, 6, 1)
    torch.manual_seed(40)
    x = st0
    for t in range(T):
        a_t = ticks.tick(x, model, pd, "average", 1)
        assert torch.equal(a_t[:, 0], acts[t]), t
        x = xs[t]
    assert torch.equal(torch.rand(1), after)  # the torch stream stands where T ticks leave it
    assert torch.equal(ep.a_mat, ticks.a_mat) and torch.equal(ep.a_seq, ticks.a_seq) and torch.equal(ep.a_seq, a_seq)
    torch.manual_seed(40)
    res = sim.simulate(st0, model, pd, T, "average", goal=[0.0, 0.0], goal_radius=0.5, plant_params=true)
    assert torch.equal(res.states, xs) and torch.equal(res.actions, acts) and res.t0 == T and not bool(res.status.any())
    assert bool((res.n_run == T).all()) and bool(torch.isfinite(res.loss).all()) and tuple(res.costs.shape) == (T, B)
    twin = copy.deepcopy(ep)  # between two episodes
    torch.manual_seed(41)
    one = ep.run_episodes(xs[-1], model, pd, 2, "argmax", plant_params=true, active=[1, 0, 1])
    torch.manual_seed(41)
    two = twin.run_episodes(xs[-1], model, pd, 2, "argmax", plant_params=true, active=[1, 0, 1])
    for u, v in zip(one, two):  # (the inactive environment's rows are NaN in both)
        assert torch.equal(torch.nan_to_num(u, nan=7.0), torch.nan_to_num(v, nan=7.0))
    assert bool(torch.isnan(one[0][:, 1]).all()) and torch.equal(ep.a_mat, twin.a_mat)


def test_pendulum_driver_runs_the_baselines_as_one_simulate():
    """run_pendulum_simulations(use_svmpc=False) against BatchDISCO.simulate called directly: the DISCO case (sigma points of dyn_dist) and
    the baseline under the exact model (every environment's true row in its rollouts)"""
    import torch.distributions as dist
    from dust_amd.controllers import BatchDISCO
    from dust_amd.costs import PendulumQuadCos
    from dust_amd.models import PendulumModel
    from dust_amd.utils.simulations import run_pendulum_simulations
    from dust_amd.utils.utf import MerweScaledUTF

    B, H, S, steps = 3, 5, 16, 4
    env, cost = PendulumModel(), PendulumQuadCos()
    pd = dist.Independent(dist.Uniform(torch.tensor([0.6, 0.6]), torch.tensor([1.3, 1.3])), 1)
    truths = [dict(length=1.2, mass=0.8), dict(length=0.7, mass=1.1), dict(length=1.0, mass=1.25)]
    true = torch.tensor([[t["length"], t["mass"]] for t in truths])
    kw = dict(temperature=20.0, a_cov=4.0 * torch.eye(1), inst_cost_fn=cost.inst_cost, term_cost_fn=cost.term_cost, seeds=[41, 42, 43])
    init = 0.3 * torch.randn(1, H, 1, generator=torch.Generator().manual_seed(2))
    st0 = torch.tensor([3.0, 0.0])
    mk = dict(g=10.0, uncertain_params=("length", "mass"))
    for exact in (False, True):
        sampling = dict(params_sampling=True, params_samples=1) if exact else dict(params_sampling=MerweScaledUTF(n=2, alpha=0.5))
        ctrl = BatchDISCO(B, env.observation_space, env.action_space, H, 1, S, **sampling, **kw)
        data = run_pendulum_simulations(st0, init, mk, truths, ctrl, None, None, None, episodes=B, steps=steps, use_svmpc=False, dyn_dist=pd,
                                        use_exact_model=exact)
        direct = copy.deepcopy(ctrl)
        direct.a_mat = init[None].repeat(B, 1, 1, 1)
        res = direct.simulate(st0.reshape(1, -1).repeat(B, 1), PendulumModel(**mk), pd, steps, "average", plant_params=true,
                              params=true[:, None, :] if exact else None)
        assert np.array_equal(data["Cost"], res.costs.numpy().T) and np.array_equal(data["Actions"], res.actions.numpy()[..., 0].T)
        assert np.array_equal(data["Position"], res.states.numpy()[..., 0].T) and data["AvgCumCost"].shape == (B, steps)
        assert np.array_equal(data["ExpParams"][:, 0], true.numpy()) and np.isfinite(data["Cost"]).all()
        assert len({tuple(r) for r in data["Actions"].tolist()}) == B  # (every environment its own plant and stream)
        assert ctrl._batch is None  # the driver runs a deep copy: the caller's controller is untouched
    with pytest.raises(ValueError):
        run_pendulum_simulations(st0, init, mk, truths, ctrl, None, None, None, episodes=2, steps=steps, use_svmpc=False)


def test_particle_driver_accepts_a_batchdisco():
    """run_particle_episodes with a `BatchDISCO` against simulate called directly with step("argmax"), the goal and the crash rule; the
    starts of tests/disco_cases.py `part`: a crash in period 0, the goal in period 0, a crash in period 1, a whole episode"""
    from dust_amd.controllers import BatchDISCO
    from dust_amd.models import Particle
    from dust_amd.utils.simulations import run_particle_episodes

    case = dc.BY_ID["part"]
    model = Particle(**dc.ac.PART_ENV, mass=2.0)
    B, steps = case["B"], 3
    kw = dict(temperature=50.0, a_cov=25.0 * torch.eye(2), inst_cost_fn=model.default_inst_cost, term_cost_fn=model.default_term_cost,
              params_sampling=None, seeds=[51, 52, 53, 54])
    ctrl = BatchDISCO(B, model.observation_space, model.action_space, 6, 2, 32, **kw)
    twin = copy.deepcopy(ctrl)
    st0 = torch.tensor(case["start"])
    loss = run_particle_episodes(st0, model, None, ctrl, steps=steps)
    res = twin.simulate(st0, model, None, steps, "argmax", goal=model.target, goal_radius=1.0, stop_on_crash=True)
    assert torch.equal(loss, res.loss) and res.status.tolist() == [2, 1, 2, 0] and res.n_run.tolist() == [1, 1, 2, 3]
    assert bool(torch.isinf(loss[[0, 2]]).all()) and bool(torch.isfinite(loss[[1, 3]]).all())
    with pytest.raises(ValueError):
        run_particle_episodes(st0, model, None, ctrl, steps=steps, mpf=object())


def test_example_runs_tiny():
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples", "pendulum_baselines_example.py")
    spec = importlib.util.spec_from_file_location("pendulum_baselines_example", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    out, true = mod.run(quiet=True, **mod.TINY)
    B, steps = mod.TINY["episodes"], mod.TINY["steps"]
    assert sorted(out) == sorted(mod.CASES) and tuple(true.shape) == (B, 2)
    for k, v in out.items():
        assert v.shape == (B, steps) and np.isfinite(v).all(), k
        assert len(set(v[:, -1].tolist())) == B, k  # every episode its own plant
