"""Closed-loop episodes on the device (csrc/svmpc_episode.hpp svmpc_episode_kernel / svmpc_skid_nav_episode_kernel,
dust_svmpc_batch_episode, `SvmpcBatch.episode`, `BatchSVMPC.run_episodes`): T periods of tick, plant step and records in ONE launch.
Every np.array_equal below is bit for bit.

1. an episode is its periods: episode(T) against T ticks of a clone fed the episode's own recorded states - first actions, particle
   weights, every getter, the last a_seq, and one further identical tick on both (counters, Philox position, optimiser state);
2. the plant: every recorded state against the float64 step of tests/amppi_cases.py on the device's OWN previous state and action, within
   the tolerance tests/svmpc_episode_cases.py measures from the restatement alone, and held away from three wrong plants;
3. episode(T1) then episode(T2) is episode(T1 + T2);
4. an environment computes the same alone, in slots 0 / 2 / 4 of five and beside inactive neighbours, which stay untouched;
5. one launch per call, every refusal before any launch;
6. `BatchSVMPC.run_episodes` against tick() under one torch seed, a deep copy between two episodes, the example.
"""
import copy
import functools
import importlib.util
import os

import numpy as np
import pytest
import torch

import svmpc_episode_cases as cases
from helpers import elemerr

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# (DUST_SVB_ACTIONS exists only behind DUST_SVMPC_BATCH_KEEP_ACTIONS, which an episode refuses with every other flag)
GETTERS = ("THETA", "PRIOR_MEANS", "PRIOR_MIX", "A_MAT", "COSTS", "SCORE", "PHI", "LOG_L", "LOG_P", "A_MIX")


def _L():
    from dust_amd import _lib

    return _lib


def _records(b):
    L = _L()
    return {n: b.get(getattr(L, "SVB_" + n)) for n in GETTERS}


def _same(x, y):
    """the getters of two batches agree bit for bit"""
    for n in GETTERS:
        assert np.array_equal(x[n], y[n]), n


def _grid(case):
    if case["family"] == "particle":
        from oracle import grid_4x4_map

        return grid_4x4_map()
    return cases.nav_map() if case["nav"] else None


def _inputs(case, T=None):
    """every environment's own start state, particles, true row, seed and dynamics samples (one more period than T: the further tick)"""
    T = case["T"] if T is None else T
    mu, th = cases.particles(case)
    return dict(st=cases.start_states(case), mu=mu, th=th, plant=cases.plant_rows(case), params=cases.tick_params(case, T + 1),
                seeds=[case["seed"] + 13 * b for b in range(case["B"])])


def _batch(case, inp, envs=None):
    """a batch whose slot k holds environment envs[k] of the case (default: all of them, in order)"""
    from dust_amd import Context

    L = _L()
    envs = list(range(case["B"])) if envs is None else list(envs)
    c = Context(grid=_grid(case), **cases.context_kwargs(case))
    b = c.svmpc_batch(len(envs), seeds=[inp["seeds"][e] for e in envs])
    c.close()
    b.set(L.SVB_THETA, inp["th"][envs])
    b.set(L.SVB_PRIOR_MEANS, inp["mu"][envs])
    b.set(L.SVB_A_MAT, inp["th"][envs])
    return b


def _sub(inp, envs, t0=0, t1=None):
    """(states, params [t0:t1], plant rows) of these environments"""
    envs = list(envs)
    return (inp["st"][envs], None if inp["params"] is None else np.ascontiguousarray(inp["params"][t0:t1][:, envs]),
            None if inp["plant"] is None else inp["plant"][envs])


@functools.lru_cache(maxsize=None)
def _run(cid):
    """the case's episode and, on a clone taken before it, its T ticks fed the recorded states; then one further tick on both"""
    case = cases.BY_ID[cid]
    T, n = case["T"], case["n_steps"]
    inp = _inputs(case)
    b = _batch(case, inp)
    twin = b.clone()
    st, params, plant = _sub(inp, range(case["B"]), 0, T)
    xs, acts, pw, a_seq = b.episode(st, T, n, params, plant)
    ticks, x = [], st
    for t in range(T):
        ticks.append(twin.tick(x, n, params=None if params is None else params[t]))
        x = xs[t]
    out = dict(inp=inp, xs=xs, acts=acts, pw=pw, a_seq=a_seq, ticks=ticks, after=(_records(b), _records(twin)))
    extra = None if inp["params"] is None else inp["params"][T]
    out["further"] = (b.tick(xs[-1], n, params=extra), twin.tick(xs[-1], n, params=extra), _records(b), _records(twin))
    b.close()
    twin.close()
    return out


# ------------------------------------------------------------------------------------------------ 1. an episode is its periods
@pytest.mark.parametrize("cid", cases.IDS)
def test_episode_equals_its_periods(cid):
    case, r = cases.BY_ID[cid], _run(cid)
    T, B, f = case["T"], case["B"], cases.family(case)
    assert r["xs"].shape == (T, B, f["ds"]) and r["acts"].shape == (T, B, f["da"]) and r["pw"].shape == (T, B, case["N"])
    assert np.isfinite(r["xs"]).all() and np.isfinite(r["acts"]).all()
    for t, (a_t, pw_t) in enumerate(r["ticks"]):
        assert np.array_equal(a_t[:, 0], r["acts"][t]), t
        assert np.array_equal(pw_t, r["pw"][t]), t
    assert np.array_equal(r["ticks"][-1][0], r["a_seq"])
    _same(*r["after"])
    (a1, p1), (a2, p2), g1, g2 = r["further"]
    assert np.array_equal(a1, a2) and np.array_equal(p1, p2)
    _same(g1, g2)
    if T > 1 and case["N"] * case["H"] > 1:  # (the periods are not copies of one another)
        assert not np.array_equal(r["acts"][0], r["acts"][1])


# ------------------------------------------------------------------------------------------------ 2. the plant
@pytest.mark.parametrize("cid", cases.IDS)
def test_plant_steps_against_float64(cid):
    """stage-wise: states_out[t] against the float64 step of (states_{t-1}, actions_out[t], the true row) - the device's own previous
    state and action, never a whole trajectory"""
    case, r = cases.BY_ID[cid], _run(cid)
    grid = _grid(case) if case["family"] == "particle" else None
    tol = cases.plant_tolerance(case, grid)
    T, rows = case["T"], r["inp"]["plant"]
    prev = np.concatenate((r["inp"]["st"][None], r["xs"][:-1]))
    ref = np.stack([cases.plant_step(case, prev[t], r["acts"][t], rows, grid) for t in range(T)])
    err = elemerr(r["xs"], ref)
    var = {}
    for t in range(T):
        for k, v in cases.variant_steps(case, prev[t], r["acts"][t], r["acts"][t - 1] if t else None, rows, grid).items():
            var.setdefault(k, []).append(v)
    far = {k: elemerr(r["xs"][T - len(v):], np.stack(v)) / tol for k, v in var.items()}
    print("%-8s plant err %.2e tol %.2e  " % (cid, err, tol) + "  ".join("%s %.0f" % kv for kv in sorted(far.items())))
    assert err < tol, (cid, err, tol)
    assert set(far) == set(cases.POWER[cid])
    for k, least in cases.POWER[cid].items():
        assert far[k] >= least, (cid, k, far[k], least)
    if cid == "part":  # environment 1 sits on an occupied cell: the plant's collision freeze holds its position
        assert np.array_equal(r["xs"][:, 1, :2], np.broadcast_to(r["inp"]["st"][1, :2], (T, 2)))
        assert not np.array_equal(r["xs"][0, 0, :2], r["inp"]["st"][0, :2])


# ------------------------------------------------------------------------------------------------ 3. concatenation
@pytest.mark.parametrize("cid", [c for c in cases.IDS if cases.BY_ID[c]["T"] > 1])
def test_two_episodes_concatenate(cid):
    case, r = cases.BY_ID[cid], _run(cid)
    T, n, envs = case["T"], case["n_steps"], range(case["B"])
    b = _batch(case, r["inp"])
    st, p1, plant = _sub(r["inp"], envs, 0, 1)
    _, p2, _ = _sub(r["inp"], envs, 1, T)
    x1, a1, w1, _ = b.episode(st, 1, n, p1, plant)
    x2, a2, w2, s2 = b.episode(x1[-1], T - 1, n, p2, plant)
    got = _records(b)
    b.close()
    assert np.array_equal(np.concatenate((x1, x2)), r["xs"]) and np.array_equal(np.concatenate((a1, a2)), r["acts"])
    assert np.array_equal(np.concatenate((w1, w2)), r["pw"]) and np.array_equal(s2, r["a_seq"])
    _same(got, r["after"][0])


# ------------------------------------------------------------------------------------------------ 4. independence from the batch
@pytest.mark.parametrize("cid", ["pend", "part", "skid_nav"])
def test_an_environment_does_not_depend_on_its_batch(cid):
    case, r = cases.BY_ID[cid], _run(cid)
    T, n, inp, e = case["T"], case["n_steps"], r["inp"], 1

    def episode(b, envs, active=None, want_pw=True):
        st, params, plant = _sub(inp, envs, 0, T)
        return b.episode(st, T, n, params, plant, active=active, want_pw=want_pw)

    want = tuple(v[:, e] for v in (r["xs"], r["acts"], r["pw"])) + (r["a_seq"][e],)
    ref = {k: v[e] for k, v in r["after"][0].items()}

    def check(out, got, slot):
        for u, v in zip(out[:3], want[:3]):
            assert np.array_equal(u[:, slot], v), slot
        assert np.array_equal(out[3][slot], want[3]), slot
        for k in GETTERS:
            assert np.array_equal(got[k][slot], ref[k]), (k, slot)

    alone = _batch(case, inp, [e])
    check(episode(alone, [e]), _records(alone), 0)
    alone.close()
    envs = [e, 0, e, (e + 1) % case["B"], e]  # slots 0 / 2 / 4 of five
    five = _batch(case, inp, envs)
    out, got = episode(five, envs), _records(five)
    five.close()
    for slot in (0, 2, 4):
        check(out, got, slot)
    envs = [0, e, 0]  # beside inactive neighbours: a tick first, so that they have getters to keep
    three = _batch(case, inp, envs)
    st, params, _ = _sub(inp, envs, 0, 1)
    lone = _batch(case, inp, [e])
    three.tick(st, n, params=None if params is None else params[0])
    lone.tick(st[1:2], n, params=None if params is None else params[0][1:2])
    before = _records(three)
    out, got = episode(three, envs, active=[0, 1, 0]), _records(three)
    solo = episode(lone, [e])
    solo_got = _records(lone)
    three.close()
    lone.close()
    for k in range(3):  # [T, 3, .] records; the neighbours' rows are never written: NaN on the host
        assert np.array_equal(out[k][:, 1], solo[k][:, 0]) and np.isnan(out[k][:, [0, 2]]).all(), k
    assert np.array_equal(out[3][1], solo[3][0]) and np.isnan(out[3][[0, 2]]).all()
    for k in GETTERS:
        assert np.array_equal(got[k][1], solo_got[k][0]), k
        assert np.array_equal(got[k][[0, 2]], before[k][[0, 2]]), k


# ------------------------------------------------------------------------------------------------ 5. plumbing
def test_one_launch_per_episode_and_refusals_before_any_launch():
    L = _L()
    case = cases.BY_ID["pend"]
    inp = _inputs(case)
    B, n = case["B"], case["n_steps"]
    b = _batch(case, inp)
    b.ctx.profile(True)
    count = lambda: b.ctx.profile_get().get("svmpc_batch_kernel", (0.0, 0))[1]
    total = lambda: sum(v[1] for v in b.ctx.profile_get().values())
    st, params, plant = _sub(inp, range(B), 0, 3)
    b.episode(st, 1, n, params[:1], plant)
    assert count() == 1 == total()
    b.episode(st, 3, n, params, plant)
    assert count() == 2 == total()
    before = _records(b)
    lib, FP = L.load(), L.FP
    f = lambda a: np.ascontiguousarray(a, np.float32)
    sp, pp, lp = f(st), f(params), f(plant)
    xs, ac, pw, sq = (np.zeros(s, np.float32) for s in ((3, B, 2), (3, B, 1), (3, B, case["N"]), (B, case["H"], 1)))
    P = lambda a: None if a is None else a.ctypes.data_as(FP)

    def call(states=sp, T=3, n_steps=n, prm=pp, plt=lp, flags=0, so=xs, ao=ac):
        return lib.dust_svmpc_batch_episode(b._h, P(states), T, n_steps, P(prm), P(plt), flags, None, P(so), P(ao), P(pw), P(sq))

    big = np.zeros((4097, B, n, case["M"], 2), np.float32)
    refused = [(call(states=None), L.ERR_INVALID), (call(so=None), L.ERR_INVALID), (call(ao=None), L.ERR_INVALID),
               (call(n_steps=0), L.ERR_INVALID), (call(T=0), L.ERR_INVALID), (call(T=4097, prm=big), L.ERR_INVALID),
               (call(prm=None), L.ERR_INVALID), (call(flags=L.SVMPC_BATCH_KEEP_ACTIONS), L.ERR_UNSUPPORTED),
               (call(flags=L.PTR_DEVICE), L.ERR_UNSUPPORTED), (call(flags=L.STORE_STATES), L.ERR_UNSUPPORTED)]
    for got, want in refused:
        assert got == want, (got, want)
    assert count() == 2 == total()
    _same(_records(b), before)
    assert not xs.any() and not ac.any() and not pw.any() and not sq.any()  # nothing was written either
    b.close()
    # dim_p = 0: neither dynamics samples nor true rows
    c0 = cases.BY_ID["one"]
    i0 = _inputs(c0)
    b0 = _batch(c0, i0)
    b0.ctx.profile(True)
    row = np.ones((1, 1, 1, 1, 1), np.float32)
    for kw in (dict(params=row), dict(plant_params=row.reshape(1, 1))):
        with pytest.raises(L.DustError) as e:
            b0.episode(i0["st"], 1, 1, **kw)
        assert e.value.status == L.ERR_INVALID
    assert sum(v[1] for v in b0.ctx.profile_get().values()) == 0
    b0.close()


# ------------------------------------------------------------------------------------------------ 6. the class
def _mirror(n_envs, seed=0, N=3, S=16, H=6, M=3):
    from dust_amd.controllers import MultiDISCO
    from dust_amd.costs import PendulumQuadCos
    from dust_amd.inference import BatchSVMPC, ExponentiatedUtility, get_gmm
    from dust_amd.kernels import RBFKernel
    from dust_amd.models import PendulumModel

    model, cost = PendulumModel(uncertain_params=("length", "mass")), PendulumQuadCos()
    ctrl = MultiDISCO(model.observation_space, model.action_space, H, N, S, temperature=1.0, a_cov=4.0 * torch.eye(1), inst_cost_fn=cost.inst_cost,
                      term_cost_fn=cost.term_cost, params_sampling=True, params_samples=M, seed=seed)
    g = torch.Generator().manual_seed(3)
    mu = torch.randn(N, H, 1, generator=g)
    th = mu + 2 * torch.randn(N, H, 1, generator=g)
    ctrl.a_mat = th.clone()
    prior = get_gmm(mu, torch.ones(N), 4.0 * torch.eye(1))
    lik = ExponentiatedUtility(alpha=1.0, n_samples=S, controller=ctrl, model=model)
    return BatchSVMPC(n_envs, init_particles=th, prior=prior, likelihood=lik, kernel=RBFKernel(), n_particles=N, n_steps=2,
                      optimizer_class=torch.optim.Adam, lr=0.1)


def test_run_episodes_against_ticks_of_the_class():
    """run_episodes(T) draws its dynamics samples as T ticks do: under the same torch seed, T calls of tick() on a deep copy, fed the
    recorded states, give the same first actions bit for bit; so does a deep copy taken between two episodes"""
    import torch.distributions as dist

    B, T = 3, 3
    pd = dist.Independent(dist.Uniform(torch.tensor([0.8, 0.8]), torch.tensor([1.2, 1.2])), 1)
    true = torch.tensor([[1.2, 0.8], [0.8, 1.1], [1.0, 1.3]])
    st0 = torch.tensor([[3.0, 0.0], [2.5, 0.2], [3.4, -0.1]])
    ep = _mirror(B)
    ep.tick(st0, pd)  # (creates the device batch, so that the deep copy below carries one)
    ticks = copy.deepcopy(ep)
    torch.manual_seed(40)
    xs, acts, pw, a_seq = ep.run_episodes(st0, pd, T, plant_params=true)
    after = torch.rand(1)
    assert all(isinstance(v, torch.Tensor) for v in (xs, acts, pw, a_seq)) and tuple(xs.shape) == (T, B, 2) and tuple(acts.shape) == (T, B, 1)
    torch.manual_seed(40)
    x = st0
    for t in range(T):
        a_t, pw_t = ticks.tick(x, pd)
        assert torch.equal(a_t[:, 0], acts[t]) and torch.equal(pw_t, pw[t]), t
        x = xs[t]
    assert torch.equal(a_t, a_seq) and torch.equal(torch.rand(1), after)  # the torch stream stands where T ticks leave it
    assert torch.equal(ep.theta, ticks.theta)
    twin = copy.deepcopy(ep)  # between two episodes
    torch.manual_seed(41)
    one = ep.run_episodes(xs[-1], pd, 2, plant_params=true, active=[1, 0, 1])
    torch.manual_seed(41)
    two = twin.run_episodes(xs[-1], pd, 2, plant_params=true, active=[1, 0, 1])
    for u, v in zip(one, two):  # (the inactive environment's rows are NaN in both)
        assert torch.equal(torch.nan_to_num(u, nan=7.0), torch.nan_to_num(v, nan=7.0))
    assert bool(torch.isnan(one[0][:, 1]).all()) and bool(torch.isnan(one[1][:, 1]).all()) and torch.equal(ep.theta, twin.theta)


def test_example_runs_tiny():
    path = os.path.join(ROOT, "examples", "svmpc_episode_example.py")
    spec = importlib.util.spec_from_file_location("svmpc_episode_example", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    avg = mod.run(quiet=True, **mod.TINY)
    assert tuple(avg.shape) == (mod.TINY["n_envs"],) and bool(torch.isfinite(avg).all()) and len(set(avg.tolist())) == mod.TINY["n_envs"]
