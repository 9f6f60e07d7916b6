"""Closed-loop AMPPI episodes on the device (csrc/amppi_episode.hpp amppi_period_kernel / amppi_skid_nav_period_kernel,
dust_amppi_batch_episode, `AmppiBatch.episode`, `BatchAMPPI.run_episodes`): T periods of tick, plant step, records and roll, one launch
per period and no host between two periods.  Every np.array_equal below is bit for bit.

1. an episode is its periods: episode(T) against T x (update of a clone fed the episode's own recorded states, then roll) - costs,
   omega, first actions, the sequences, get_actions, and one further identical tick on both (the Philox position);
2. the plant: every recorded state against the float64 step of tests/amppi_cases.py on the device's OWN previous state and action, within
   the tolerance tests/amppi_episode_cases.py measures from the restatement alone, and held away from three wrong plants;
3. episode(1) then episode(T - 1) is episode(T);
4. an environment computes the same alone, in slots 0 / 2 / 4 of five, beside inactive neighbours, which stay untouched, and from a
   clone taken between two episodes;
5. T launches per call, every refusal before any launch;
6. `BatchAMPPI.run_episodes` against update_actions + roll under one torch seed, the example.
"""
import copy
import functools
import importlib.util
import os

import numpy as np
import pytest
import torch

import amppi_cases as ac
import amppi_episode_cases as cases
from helpers import elemerr

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _L():
    from dust_amd import _lib

    return _lib


def _grid(case):
    if case["family"] == "particle":
        from oracle import grid_4x4_map

        return grid_4x4_map()
    return cases.nav_map() if case["nav"] else None


def _inputs(case):
    """every environment's own start state, sequence, true row, seed and parameter rows (one more period than T: the further tick)"""
    return dict(st=cases.start_states(case), a0=cases.start_sequences(case), plant=cases.plant_rows(case),
                params=cases.tick_params(case, case["T"] + 1), seeds=[case["seed"] + 13 * b for b in range(case["B"])])


def _batch(case, inp, envs=None):
    """a batch whose slot k holds environment envs[k] of the case (default: all of them, in order)"""
    from dust_amd import Context

    envs = list(range(case["B"])) if envs is None else list(envs)
    if case["map_dev"]:  # the development switch is read when a context is created: the prototype and the batch's own copy of it
        os.environ["DUST_NAV_GRID_HBM"] = "1"
    try:
        c = Context(grid=_grid(case), **cases.context_kwargs(case))
        if case["mode"] == "ut":
            c.set_param_weights(np.asarray(ac.weights(len(case["up"]))[0], np.float32))
        b = c.amppi_batch(len(envs), [inp["seeds"][e] for e in envs])
        c.close()
    finally:
        os.environ.pop("DUST_NAV_GRID_HBM", None)
    b.set_a_seq(inp["a0"][envs])
    return b


def _sub(inp, envs, t0=0, t1=None):
    """(states, params [t0:t1], plant rows) of these environments"""
    envs = list(envs)
    return (inp["st"][envs], None if inp["params"] is None else np.ascontiguousarray(inp["params"][t0:t1][:, envs]),
            None if inp["plant"] is None else inp["plant"][envs])


def _kw(case):
    return dict(shared_params=case["mode"] == "single")


@functools.lru_cache(maxsize=None)
def _run(cid):
    """the case's episode and, on a clone taken before it, its T updates fed the recorded states, each followed by the roll; then one
    further tick on both"""
    case = cases.BY_ID[cid]
    T, roll = case["T"], case["roll_steps"]
    inp = _inputs(case)
    b = _batch(case, inp)
    twin = b.clone()
    st, params, plant = _sub(inp, range(case["B"]), 0, T)
    xs, acts, costs, omega, a_seq = b.episode(st, T, params, plant_params=plant, roll_steps=roll, **_kw(case))
    ticks, x = [], st
    for t in range(T):
        c_t, o_t, s_t, _ = twin.update(x, None, None if params is None else params[t], **_kw(case))
        drawn = twin.get_actions()
        twin.roll(roll)
        ticks.append((c_t, o_t, s_t, drawn, twin.get_a_seq()))
        x = xs[t]
    out = dict(inp=inp, xs=xs, acts=acts, costs=costs, omega=omega, a_seq=a_seq, ticks=ticks,
               after=((b.get_a_seq(), b.get_actions()), (twin.get_a_seq(), twin.get_actions())))
    extra = None if inp["params"] is None else inp["params"][T]
    out["further"] = (b.update(xs[-1], None, extra, want_actions=True, **_kw(case)), twin.update(xs[-1], None, extra, want_actions=True, **_kw(case)))
    b.close()
    twin.close()
    return out


# ------------------------------------------------------------------------------------------------ 1. an episode is its periods
@pytest.mark.parametrize("cid", cases.IDS)
def test_episode_equals_its_periods(cid):
    case, r = cases.BY_ID[cid], _run(cid)
    T, B, S, f = case["T"], case["B"], case["S"], cases.family(case)
    assert r["xs"].shape == (T, B, f["ds"]) and r["acts"].shape == (T, B, f["da"]) and r["costs"].shape == (T, B, S) == r["omega"].shape
    for v in (r["xs"], r["acts"], r["costs"], r["omega"], r["a_seq"]):
        assert np.isfinite(v).all()
    for t, (c_t, o_t, s_t, _, _) in enumerate(r["ticks"]):
        assert np.array_equal(c_t, r["costs"][t]), t
        assert np.array_equal(o_t, r["omega"][t]), t
        assert np.array_equal(s_t[:, 0], r["acts"][t]), t
    assert np.array_equal(r["ticks"][-1][2], r["a_seq"])  # the last period's sequence before its roll
    (s1, g1), (s2, g2) = r["after"]
    assert np.array_equal(s1, s2) and np.array_equal(s1, r["ticks"][-1][4]) and np.array_equal(g1, g2)
    shift = min(case["roll_steps"], case["H"])
    assert np.array_equal(s1[:, :case["H"] - shift], r["a_seq"][:, shift:]) and not s1[:, case["H"] - shift:].any()
    for u, v in zip(*r["further"]):
        assert np.array_equal(u, v)
    if T > 1 and S > 1:  # (the periods are not copies of one another)
        assert not np.array_equal(r["costs"][0], r["costs"][1]) and not np.array_equal(r["ticks"][0][3], r["ticks"][1][3])
    for b in range(1, B):  # (nor the environments)
        assert not np.array_equal(r["xs"][:, 0], r["xs"][:, b])


# ------------------------------------------------------------------------------------------------ 2. the plant
@pytest.mark.parametrize("cid", cases.IDS)
def test_plant_steps_against_float64(cid):
    """stage-wise: states_out[t] against the float64 step of (states_{t-1}, actions_out[t], the true row) - the device's own previous
    state and action, never a whole trajectory - and at least POWER tolerances from every wrong plant in at least one period"""
    case, r = cases.BY_ID[cid], _run(cid)
    grid = _grid(case) if case["family"] == "particle" else None
    tol = cases.plant_tolerance(case, grid)
    T, rows = case["T"], r["inp"]["plant"]
    prev = np.concatenate((r["inp"]["st"][None], r["xs"][:-1]))
    ref = np.stack([cases.plant_step(case, prev[t], r["acts"][t], rows, grid) for t in range(T)])
    err = elemerr(r["xs"], ref)
    far = cases.distances(case, r["xs"], prev, r["acts"], rows, grid, tol)
    print("%-10s plant err %.2e tol %.2e  " % (cid, err, tol) + "  ".join("%s %.0f" % kv for kv in sorted(far.items())))
    assert err < tol, (cid, err, tol)
    assert set(far) == cases.variants_of(case)
    for k, v in far.items():
        assert v >= cases.POWER, (cid, k, v)
    if cid == "part":  # environment 1 sits on an occupied cell: the plant's collision freeze holds its position
        assert np.array_equal(r["xs"][:, 1, :2], np.broadcast_to(r["inp"]["st"][1, :2], (T, 2)))
        assert not np.array_equal(r["xs"][0, 0, :2], r["inp"]["st"][0, :2])


def test_both_map_paths_give_the_same_bits():
    a, b = _run("nav_lds"), _run("nav_dev")
    for k in ("xs", "acts", "costs", "omega", "a_seq"):
        assert np.array_equal(a[k], b[k]), k


# ------------------------------------------------------------------------------------------------ 3. concatenation
@pytest.mark.parametrize("cid", [c for c in cases.IDS if cases.BY_ID[c]["T"] > 1])
def test_two_episodes_concatenate(cid):
    case, r = cases.BY_ID[cid], _run(cid)
    T, envs, roll = case["T"], range(case["B"]), case["roll_steps"]
    b = _batch(case, r["inp"])
    st, p1, plant = _sub(r["inp"], envs, 0, 1)
    _, p2, _ = _sub(r["inp"], envs, 1, T)
    one = b.episode(st, 1, p1, plant_params=plant, roll_steps=roll, **_kw(case))
    two = b.episode(one[0][-1], T - 1, p2, plant_params=plant, roll_steps=roll, **_kw(case))
    got = (b.get_a_seq(), b.get_actions())
    b.close()
    for k, name in enumerate(("xs", "acts", "costs", "omega")):
        assert np.array_equal(np.concatenate((one[k], two[k])), r[name]), name
    assert np.array_equal(two[4], r["a_seq"])
    assert np.array_equal(got[0], r["after"][0][0]) and np.array_equal(got[1], r["after"][0][1])


# ------------------------------------------------------------------------------------------------ 4. independence from the batch
@pytest.mark.parametrize("cid", ["s257_edge", "part", "nav_lds", "s1021_ut"])
def test_an_environment_does_not_depend_on_its_batch(cid):
    case, r = cases.BY_ID[cid], _run(cid)
    T, inp, e, roll = case["T"], r["inp"], 1, case["roll_steps"]

    def episode(b, envs, active=None, t0=0, t1=T, states=None):
        st, params, plant = _sub(inp, envs, t0, t1)
        return b.episode(st if states is None else states, t1 - t0, params, plant_params=plant, active=active, roll_steps=roll, **_kw(case))

    want = tuple(r[k][:, e] for k in ("xs", "acts", "costs", "omega")) + (r["a_seq"][e],)
    ref = tuple(v[e] for v in r["after"][0])

    def check(out, b, slot):
        for u, v in zip(out[:4], want[:4]):
            assert np.array_equal(u[:, slot], v), slot
        assert np.array_equal(out[4][slot], want[4]), slot
        assert np.array_equal(b.get_a_seq()[slot], ref[0]) and np.array_equal(b.get_actions()[slot], ref[1]), slot

    alone = _batch(case, inp, [e])
    check(episode(alone, [e]), alone, 0)
    alone.close()
    envs = [e, 0, e, (e + 1) % case["B"], e]  # slots 0 / 2 / 4 of five
    five = _batch(case, inp, envs)
    out = episode(five, envs)
    for slot in (0, 2, 4):
        check(out, five, slot)
    five.close()
    envs = [0, e, 0]  # beside inactive neighbours: a tick first, so that they have actions to keep
    three = _batch(case, inp, envs)
    st, params, _ = _sub(inp, envs, 0, 1)
    three.update(st, None, None if params is None else params[0], **_kw(case))
    three.set_a_seq(inp["a0"][envs])
    before = (three.get_a_seq(), three.get_actions())
    out = episode(three, envs, active=[0, 1, 0])
    after = (three.get_a_seq(), three.get_actions())
    # the neighbours' stream positions have not moved either: their next tick is that of a lone batch that never saw the episode
    first = None if params is None else params[0]
    ref0 = _batch(case, inp, [0])
    ref0.update(st[:1], None, None if first is None else first[:1], **_kw(case))
    ref0.set_a_seq(inp["a0"][[0]])
    nxt, want0 = three.update(st, None, first, **_kw(case)), ref0.update(st[:1], None, None if first is None else first[:1], **_kw(case))
    ref0.close()
    for k in range(3):
        assert np.array_equal(nxt[k][0], want0[k][0]) and np.array_equal(nxt[k][2], want0[k][0]), k
    three.close()
    for k in range(4):  # [T, 3, .] records; the neighbours' rows are never written: NaN on the host
        assert np.isnan(out[k][:, [0, 2]]).all(), k
    assert np.isnan(out[4][[0, 2]]).all()
    assert np.array_equal(before[0][[0, 2]], after[0][[0, 2]])  # the neighbours' sequences have not moved
    assert np.isnan(after[1][[0, 2]]).all()  # (get_actions shows the environments of the last call, as after a masked tick)
    # (the active one drew one tick's noise before the episode: it continues its stream, as a lone batch that made the same calls)
    lone = _batch(case, inp, [e])
    lone.update(st[1:2], None, None if params is None else params[0][1:2], **_kw(case))
    lone.set_a_seq(inp["a0"][[e]])
    solo = episode(lone, [e])
    for k in range(4):
        assert np.array_equal(out[k][:, 1], solo[k][:, 0]), k
    assert np.array_equal(out[4][1], solo[4][0]) and np.array_equal(after[0][1], lone.get_a_seq()[0]) and np.array_equal(after[1][1], lone.get_actions()[0])
    lone.close()
    if T > 1:  # a clone taken between two episodes finishes as the original does
        b = _batch(case, inp)
        first = episode(b, range(case["B"]), t0=0, t1=1)
        twin = copy.deepcopy(b)
        x, y = (episode(v, range(case["B"]), t0=1, t1=T, states=first[0][-1]) for v in (b, twin))
        for u, v, name in zip(x, y, ("xs", "acts", "costs", "omega")):
            assert np.array_equal(u, v) and np.array_equal(u, r[name][1:]), name
        assert np.array_equal(b.get_a_seq(), twin.get_a_seq()) and np.array_equal(b.get_actions(), twin.get_actions())
        b.close()
        twin.close()


# ------------------------------------------------------------------------------------------------ 5. plumbing
def test_t_launches_per_episode_and_refusals_before_any_launch():
    L = _L()
    case = cases.BY_ID["s255"]
    inp = _inputs(case)
    B, S, H = case["B"], case["S"], case["H"]
    b = _batch(case, inp)
    b.ctx.profile(True)
    count = lambda: b.ctx.profile_get().get("amppi_kernel", (0.0, 0))[1]
    total = lambda: sum(v[1] for v in b.ctx.profile_get().values())
    st, params, plant = _sub(inp, range(B), 0, 3)
    b.episode(st, 1, params[:1], plant_params=plant)
    assert count() == 1 == total()
    b.episode(st, 3, params, plant_params=plant, active=[1, 0, 1])
    assert count() == 4 == total()  # T launches of the period kernel, no roll launch
    before = (b.get_a_seq(), b.get_actions())
    lib, FP = L.load(), L.FP
    f = lambda a: np.ascontiguousarray(a, np.float32)
    sp, pp, lp = f(st), f(params), f(plant)
    xs, ac_, co, om, sq = (np.zeros(s, np.float32) for s in ((3, B, 2), (3, B, 1), (3, B, S), (3, B, S), (B, H, 1)))
    P = lambda a: None if a is None else a.ctypes.data_as(FP)

    def call(states=sp, T=3, prm=pp, plt=lp, flags=0, roll=1, so=xs, ao=ac_):
        return lib.dust_amppi_batch_episode(b._h, P(states), T, P(prm), flags, roll, P(plt), None, P(so), P(ao), P(co), P(om), P(sq))

    refused = [(call(states=None), L.ERR_INVALID), (call(so=None), L.ERR_INVALID), (call(ao=None), L.ERR_INVALID),
               (call(T=0), L.ERR_INVALID), (call(T=4097), L.ERR_INVALID), (call(roll=0), L.ERR_INVALID),
               (call(flags=L.PTR_DEVICE), L.ERR_UNSUPPORTED), (call(flags=L.STORE_STATES), L.ERR_UNSUPPORTED),
               (call(flags=L.EPS_F16), L.ERR_UNSUPPORTED), (call(flags=L.STORE_F16), L.ERR_UNSUPPORTED),
               (lib.dust_amppi_batch_episode(None, P(sp), 3, P(pp), 0, 1, P(lp), None, P(xs), P(ac_), P(co), P(om), P(sq)), L.ERR_INVALID)]
    for got, want in refused:
        assert got == want, (got, want)
    assert count() == 4 == total()
    after = (b.get_a_seq(), b.get_actions())
    # (get_actions: the masked call's inactive environment shows NaN rows on both sides)
    assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1], equal_nan=True) and not np.isnan(after[1][[0, 2]]).any()
    assert not xs.any() and not ac_.any() and not co.any() and not om.any() and not sq.any()  # nothing was written either
    b.close()
    # dim_p = 0: neither parameter rows nor true rows; sigma weights without rows
    c0 = cases.BY_ID["s1"]
    i0 = _inputs(c0)
    b0 = _batch(c0, i0)
    b0.ctx.profile(True)
    for kw in (dict(params=np.ones((1, c0["B"], 1, 1), np.float32), shared_params=True), dict(plant_params=np.ones((c0["B"], 1), np.float32))):
        with pytest.raises(L.DustError) as e:
            b0.episode(i0["st"], 1, **kw)
        assert e.value.status == L.ERR_INVALID
    assert sum(v[1] for v in b0.ctx.profile_get().values()) == 0
    b0.close()
    cu = cases.BY_ID["s1021_ut"]
    iu = _inputs(cu)
    bu = _batch(cu, iu)
    bu.ctx.profile(True)
    with pytest.raises(L.DustError, match="sigma-point weights are set") as e:
        bu.episode(iu["st"], 1)
    assert e.value.status == L.ERR_INVALID and sum(v[1] for v in bu.ctx.profile_get().values()) == 0
    bu.close()


# ------------------------------------------------------------------------------------------------ 6. the class
def _mirror(n_envs, mode="extended", S=65, H=8):
    from dust_amd.controllers import BatchAMPPI
    from dust_amd.costs import PendulumQuadCos
    from dust_amd.models import PendulumModel

    import torch.distributions as dist

    model, cost = PendulumModel(uncertain_params=("length", "mass")), PendulumQuadCos()
    model.params_dist = dist.Independent(dist.Uniform(torch.tensor([0.8, 0.8]), torch.tensor([1.2, 1.2])), 1)
    g = torch.Generator().manual_seed(3)
    ctrl = BatchAMPPI(n_envs, model.observation_space, model.action_space, H, S, lambda_=100.0, a_cov=4.0 * torch.eye(1),
                      inst_cost_fn=cost.inst_cost, term_cost_fn=cost.term_cost, params_sampling=mode, init_actions=0.5 * torch.randn(H, 1, generator=g),
                      seeds=[5, 6, 7][:n_envs])
    ctrl.return_rollouts = False
    return ctrl, model


@pytest.mark.parametrize("mode", ["extended", "single"])
def test_run_episodes_against_update_actions_and_roll(mode):
    """run_episodes(T) draws its parameter rows as T calls of update_actions do: under the same torch seed, T x (update_actions, roll)
    on a deep copy, fed the recorded states, give the same costs, weights and first actions bit for bit, and the torch stream stands
    where they leave it; inactive environments draw nothing and come back as NaN"""
    B, T = 3, 3
    true = torch.tensor([[1.2, 0.8], [0.8, 1.1], [1.0, 1.3]])
    st0 = torch.tensor([[3.0, 0.0], [2.5, 0.2], [3.4, -0.1]])
    ep, model = _mirror(B, mode)
    ep.update_actions(model, st0)  # (creates the device batch, so that the deep copy below carries one)
    ep.roll(1)
    ticks = copy.deepcopy(ep)
    torch.manual_seed(40)
    xs, acts, costs, omega = ep.run_episodes(model, st0, T, plant_params=true, roll_steps=2)
    after = torch.rand(1)
    assert all(isinstance(v, torch.Tensor) for v in (xs, acts, costs, omega)) and tuple(xs.shape) == (T, B, 2) and tuple(acts.shape) == (T, B, 1)
    torch.manual_seed(40)
    x = st0
    for t in range(T):
        c_t, _, _, o_t = ticks.update_actions(model, x)
        assert torch.equal(c_t, costs[t]) and torch.equal(o_t, omega[t]) and torch.equal(ticks.a_seq[:, 0], acts[t]), t
        ticks.roll(2)
        x = xs[t]
    assert torch.equal(torch.rand(1), after) and torch.equal(ep.a_seq, ticks.a_seq)
    torch.manual_seed(41)
    one = ep.run_episodes(model, xs[-1], 2, plant_params=true, active=[1, 0, 1])
    torch.manual_seed(41)
    x = xs[-1]
    for t in range(2):
        c_t, _, _, o_t = ticks.update_actions(model, x, active=[1, 0, 1])
        assert torch.equal(torch.nan_to_num(c_t, nan=7.0), torch.nan_to_num(one[2][t], nan=7.0)), t
        ticks.roll(1, active=[1, 0, 1])
        x = torch.where(torch.isnan(one[0][t]), x, one[0][t])
    assert all(bool(torch.isnan(v[:, 1]).all()) for v in one) and torch.equal(ep.a_seq, ticks.a_seq)


def test_example_runs_tiny():
    path = os.path.join(ROOT, "examples", "amppi_episode_example.py")
    spec = importlib.util.spec_from_file_location("amppi_episode_example", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    avg = mod.run(quiet=True, **mod.TINY)
    assert tuple(avg.shape) == (mod.TINY["n_envs"],) and bool(torch.isfinite(avg).all()) and len(set(avg.tolist())) == mod.TINY["n_envs"]
