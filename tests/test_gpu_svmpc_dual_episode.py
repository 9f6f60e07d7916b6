"""DuSt-MPC episodes on the device (dust_svmpc_dual_batch_episode, csrc/svmpc_episode.hpp svmpc_dual_period_kernel,
`SvmpcBatch.dual_episode`, `BatchDualSVMPC.run_episodes`): per period the filters' update, the tick and the plant, chained on one stream.
Every np.array_equal below is bit for bit; the cases and why each exists are in tests/svmpc_dual_episode_cases.py.

1. an episode equals its periods: episode(T) against T calls of dust_svmpc_dual_batch_tick on clones of both batches, fed the episode's
   recorded states and actions - first actions, particle weights, bandwidths per period; every getter of the SVMPC batch, the filters'
   particles, prior bandwidths and statistics afterwards; then ONE further dual tick on both pairs with the pending pair (the filters'
   host rows - observations, past action, step counts - show there);
2. the plant: every recorded state against the float64 step of tests/svmpc_episode_cases.py on the device's OWN previous state and action
   under the true rows, within that file's tolerance, and held FACTOR tolerances from three wrong plants in at least one period;
3. episode(T1) then episode(T - T1), chained through the pending pair, is episode(T), for T1 = 1 and T1 = T - 1;
4. an environment computes the same alone, in slots 0 / 2 / 4 of five, beside inactive neighbours (which stay untouched on both sides) and
   from clones of both batches taken after a first episode;
5. T tick launches per call, a filter-side launch count that does not depend on B, every refusal before anything is staged or launched;
6. `BatchDualSVMPC.run_episodes` against a deep copy driven by tick(); 7. the example.
"""
import copy
import functools
import importlib.util
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import svmpc_dual_episode_cases as cases
import svmpc_episode_cases as ec
from helpers import elemerr

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# (DUST_SVB_ACTIONS exists only behind DUST_SVMPC_BATCH_KEEP_ACTIONS, which an episode refuses with every other flag)
GETTERS = ("THETA", "PRIOR_MEANS", "PRIOR_MIX", "A_MAT", "COSTS", "SCORE", "PHI", "LOG_L", "LOG_P", "A_MIX")
SETTABLE = ("THETA", "PRIOR_MEANS", "PRIOR_MIX", "A_MAT")


@pytest.fixture(autouse=True)
def _single_workgroup_filters(monkeypatch):
    """(the switch is read in dust_mpf_create; the batched filter kernels do not depend on it)"""
    monkeypatch.setenv("DUST_MPF_GRID", "0")


def _L():
    from dust_amd import _lib

    return _lib


def _grid(case):
    if case["family"] == "particle":
        from oracle import grid_4x4_map

        return grid_4x4_map()
    return None


def _state(sb, mb, names=GETTERS):
    """what both batches show of themselves"""
    L = _L()
    out = {n: sb.get(getattr(L, "SVB_" + n)) for n in names}
    out["mpf_particles"], out["mpf_prior_bw"] = mb.get_particles(), mb.get_prior_bw()
    return out


def _same(x, y, rows=None):
    assert set(x) == set(y)
    for n in x:
        u, v = (x[n], y[n]) if rows is None else (x[n][rows[0]], y[n][rows[1]])
        assert np.array_equal(u, v), n


def _setup(case, envs=None):
    """-> (controller batch, filter batch): slot k holds environment envs[k] of the case (default: all of them, in order) - its own
    particles, prior means, noise seed, filter particles and first observation"""
    from dust_amd import Context, MpfContext

    L = _L()
    envs = list(range(case["B"])) if envs is None else list(envs)
    f = ec.family(case)
    c = Context(grid=_grid(case), **ec.context_kwargs(case))
    sb = c.svmpc_batch(len(envs), seeds=[case["seed"] + 13 * e for e in envs])
    c.close()
    mu, th = ec.particles(case)
    sb.set(L.SVB_THETA, th[envs])
    sb.set(L.SVB_PRIOR_MEANS, mu[envs])
    sb.set(L.SVB_A_MAT, th[envs])
    x, st = cases.filter_particles(case)[envs], ec.start_states(case)[envs]
    kw = dict(model=f["model"], uncertain_params=case["up"], obs_std=0.2, lr=1e-3, init_bw=0.05, optimizer=case["filt_opt"], log_space=case["log"],
              dt=f["dt"])
    if case["family"] == "particle":
        kw.update(grid=_grid(case), mass=f["defaults"]["mass"])
    m = MpfContext(x[0], st[0], **kw)
    mb = m.batch(len(envs))
    m.close()
    mb.set_particles(x)
    mb.set_obs(st)
    return sb, mb


def _inputs(case, envs=None):
    """(start states, actions_prev or None, true rows for the device, seeds [T + 1, B]: one more row than T, for the further tick)"""
    envs = list(range(case["B"])) if envs is None else list(envs)
    ap = cases.first_actions(case)
    return (ec.start_states(case)[envs], None if ap is None else ap[envs], cases.device_rows(case)[envs],
            np.ascontiguousarray(cases.prior_seeds(case, case["T"] + 1)[:, envs]))


def _episode(case, sb, mb, st, ap, rows, seeds, T=None, active=None):
    T = len(seeds) if T is None else T
    return sb.dual_episode(mb, st, T, case["n_steps"], ap, mpf_steps=case["mpf_steps"], mpf_bw=case["mpf_bw"], seeds=seeds[:T], plant_params=rows,
                           active=active)


def _tick(case, sb, mb, st, ap, seeds_row, active=None):
    a_seq, pw, _, bw = sb.dual_tick(mb, st, ap, n_steps=case["n_steps"], mpf_steps=case["mpf_steps"], mpf_bw=case["mpf_bw"], seeds=seeds_row,
                                    active=active)
    return a_seq, pw, bw


@functools.lru_cache(maxsize=None)
def _run(cid):
    """the case's episode and, on clones of both batches taken before it, its T dual ticks fed the recorded states and actions; then one
    further dual tick on both pairs with the pending pair.  Computed once, shared, and left unchanged."""
    case = cases.BY_ID[cid]
    T = case["T"]
    st, ap, rows, seeds = _inputs(case)
    sb, mb = _setup(case)
    before = mb.get_particles()
    sb2, mb2 = sb.clone(), mb.clone()
    s0, s02 = mb.stats(), mb2.stats()
    xs, acts, pw, bw, a_seq = _episode(case, sb, mb, st, ap, rows, seeds, T)
    ticks, x, a = [], st, ap
    for t in range(T):
        ticks.append(_tick(case, sb2, mb2, x, a, seeds[t]))
        x, a = xs[t], acts[t]
    s1, s12 = mb.stats(), mb2.stats()
    stale = None
    if T > 1:  # the power of the comparison: the same ticks, but every update sees the FIRST state again - the filters end elsewhere
        sb3, mb3 = _setup(case)
        a = ap
        for t in range(T):
            _tick(case, sb3, mb3, st, a, seeds[t])
            a = acts[t]
        stale = mb3.get_particles()
        sb3.close()
        mb3.close()
    out = dict(st=st, ap=ap, rows=rows, seeds=seeds, xs=xs, acts=acts, pw=pw, bw=bw, a_seq=a_seq, ticks=ticks, before=before,
               stale=stale, after=(_state(sb, mb), _state(sb2, mb2)), stats=({k: s1[k] - s0[k] for k in s0}, {k: s12[k] - s02[k] for k in s02}))
    out["further"] = (_tick(case, sb, mb, xs[-1], acts[-1], seeds[T]), _tick(case, sb2, mb2, xs[-1], acts[-1], seeds[T]),
                      _state(sb, mb), _state(sb2, mb2))
    for h in (sb, mb, sb2, mb2):
        h.close()
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


# ------------------------------------------------------------------------------------------------ 1. an episode equals its periods
@pytest.mark.parametrize("cid", cases.IDS)
def test_episode_equals_its_periods(cid):
    case, r = cases.BY_ID[cid], _run(cid)
    T, B, f = case["T"], case["B"], ec.family(case)
    assert r["xs"].shape == (T, B, f["ds"]) and r["acts"].shape == (T, B, f["da"]) and r["pw"].shape == (T, B, case["N"]) and r["bw"].shape == (T, B)
    assert np.isfinite(r["xs"]).all() and np.isfinite(r["acts"]).all() and np.isfinite(r["bw"]).all()
    for t, (a_t, pw_t, bw_t) in enumerate(r["ticks"]):
        assert np.array_equal(a_t[:, 0], r["acts"][t]), t
        assert np.array_equal(pw_t, r["pw"][t]), t
        assert np.array_equal(bw_t, r["bw"][t]), t
        updated = t > 0 or case["first"]
        assert ((r["bw"][t] > 0) == updated).all(), t  # (0 where no update ran)
        if updated and case["mpf_bw"] is not None:
            assert (r["bw"][t] == np.float32(case["mpf_bw"])).all()
    assert np.array_equal(r["ticks"][-1][0], r["a_seq"])
    _same(*r["after"])
    assert r["stats"][0] == r["stats"][1] and r["stats"][0]["calls"] == T
    updates = T - (0 if case["first"] else 1)
    assert r["stats"][0]["launches"] == updates * (1 if case["mpf_bw"] is not None else 2)
    (a1, p1, b1), (a2, p2, b2), g1, g2 = r["further"]  # the pending pair, folded in by a dual tick on both sides
    assert np.array_equal(a1, a2) and np.array_equal(p1, p2) and np.array_equal(b1, b2)
    _same(g1, g2)
    if updates:  # the filters moved (no update is a fixed point), and so did the further one
        assert not np.array_equal(r["after"][0]["mpf_particles"], r["before"])
    assert not np.array_equal(g1["mpf_particles"], r["after"][0]["mpf_particles"])
    if T > 1 and case["N"] * case["H"] > 1:  # (the periods are not copies of one another)
        assert not np.array_equal(r["acts"][0], r["acts"][1])
    if T > 1:  # a stale observation changes bits, in every environment whose plant moves
        for b in range(B):
            assert np.array_equal(r["stale"][b], r["after"][0]["mpf_particles"][b]) == (cases.FROZEN.get(cid) == b), b


# ------------------------------------------------------------------------------------------------ 2. the plant
@pytest.mark.parametrize("cid", cases.IDS)
def test_plant_steps_against_float64(cid):
    """stage-wise: states_out[t] against the float64 step of (states_{t-1}, actions_out[t], the true row) - the device's own previous
    state and action, never a whole trajectory"""
    case, r = cases.BY_ID[cid], _run(cid)
    grid = _grid(case)
    tol = cases.plant_tolerance(case, grid)
    T, rows = case["T"], cases.true_rows(case)
    prev = np.concatenate((r["st"][None], r["xs"][:-1]))
    ref = np.stack([ec.plant_step(case, prev[t], r["acts"][t], rows, grid) for t in range(T)])
    err = max(elemerr(r["xs"][t], ref[t]) for t in range(T))
    far = cases.variant_distances(case, prev, r["acts"], r["xs"], tol, grid)
    print("%-22s plant err %.2e tol %.2e  " % (cid, err, tol) + "  ".join("%s %.0f" % kv for kv in sorted(far.items())))
    assert err < tol, (cid, err, tol)
    assert set(far) == ({"nominal", "unstepped"} | ({"prev_action"} if T > 1 else set()))
    for k, v in far.items():
        assert v >= cases.FACTOR, (cid, k, v)
    if cid in cases.FROZEN:  # on an occupied cell: the plant's collision freeze holds the whole state
        e = cases.FROZEN[cid]
        assert np.array_equal(r["xs"][:, e], np.broadcast_to(r["st"][e], (T, r["st"].shape[1])))
        assert not np.array_equal(r["xs"][0, 0], r["st"][0])


# ------------------------------------------------------------------------------------------------ 3. concatenation
@pytest.mark.parametrize("cid", [c for c in cases.IDS if cases.BY_ID[c]["T"] > 1])
def test_two_episodes_concatenate(cid):
    case, r = cases.BY_ID[cid], _run(cid)
    T = case["T"]
    for T1 in sorted({1, T - 1}):
        sb, mb = _setup(case)
        one = _episode(case, sb, mb, r["st"], r["ap"], r["rows"], r["seeds"][:T1])
        two = _episode(case, sb, mb, one[0][-1], one[1][-1], r["rows"], r["seeds"][T1:T])  # the pending pair: (states, actions_prev)
        got = _state(sb, mb)
        more = _tick(case, sb, mb, two[0][-1], two[1][-1], r["seeds"][T])
        sb.close()
        mb.close()
        for k, name in enumerate(("xs", "acts", "pw", "bw")):
            assert np.array_equal(np.concatenate((one[k], two[k])), r[name]), (T1, name)
        assert np.array_equal(two[4], r["a_seq"]), T1
        _same(got, r["after"][0])
        for u, v in zip(more, r["further"][0]):  # (and the filters' host rows stand where one episode leaves them)
            assert np.array_equal(u, v), T1


# ------------------------------------------------------------------------------------------------ 4. independence from the batch
@pytest.mark.parametrize("cid", ["pend_sgd_silverman", "part_mass_grid"])
def test_an_environment_does_not_depend_on_its_batch(cid):
    case, r = cases.BY_ID[cid], _run(cid)
    T, e = case["T"], 2
    want = tuple(r[k][:, e] for k in ("xs", "acts", "pw", "bw")) + (r["a_seq"][e],)
    ref = {k: v[e] for k, v in r["after"][0].items()}

    def check(out, got, slot):
        for u, v in zip(out[:4], want[:4]):
            assert np.array_equal(u[:, slot], v), slot
        assert np.array_equal(out[4][slot], want[4]), slot
        for k in ref:
            assert np.array_equal(got[k][slot], ref[k]), (k, slot)

    def again(sb, mb, out, envs, active=None):
        """a second episode of two periods from the pending pair, under the further seeds"""
        seeds2 = np.ascontiguousarray(cases.prior_seeds(case, T + 2)[T:, envs])
        return _episode(case, sb, mb, np.nan_to_num(out[0][-1]), np.nan_to_num(out[1][-1]), _inputs(case, envs)[2], seeds2, active=active)

    # alone
    st, ap, rows, seeds = _inputs(case, [e])
    sb, mb = _setup(case, [e])
    out = _episode(case, sb, mb, st, ap, rows, seeds, T)
    check(out, _state(sb, mb), 0)
    second = again(sb, mb, out, [e])
    second_state = _state(sb, mb)
    sb.close()
    mb.close()
    # slots 0 / 2 / 4 of five; then clones of both batches taken after that first episode
    envs = [e, 0, e, 1, e]
    st, ap, rows, seeds = _inputs(case, envs)
    sb, mb = _setup(case, envs)
    out = _episode(case, sb, mb, st, ap, rows, seeds, T)
    got = _state(sb, mb)
    for slot in (0, 2, 4):
        check(out, got, slot)
    sb2, mb2 = sb.clone(), mb.clone()
    for pair in ((sb, mb), (sb2, mb2)):
        s2 = again(pair[0], pair[1], out, envs)
        g2 = _state(*pair)
        for slot in (0, 2, 4):
            for u, v in zip(s2[:4], second[:4]):
                assert np.array_equal(u[:, slot], v[:, 0]), slot
            assert np.array_equal(s2[4][slot], second[4][0])
            _same(g2, second_state, rows=(slot, 0))
        pair[0].close()
        pair[1].close()
    # beside inactive neighbours: they keep everything on BOTH sides, and their record rows are not written (the NaN the binding fills in)
    envs, active = [0, e, 1], [0, 1, 0]
    st, ap, rows, seeds = _inputs(case, envs)
    sb, mb = _setup(case, envs)
    before = _state(sb, mb, SETTABLE)
    out = _episode(case, sb, mb, st, ap, rows, seeds, T, active=active)
    got = _state(sb, mb)
    for u, v in zip(out[:4], want[:4]):
        assert np.array_equal(u[:, 1], v) and np.isnan(u[:, [0, 2]]).all()
    assert np.array_equal(out[4][1], want[4]) and np.isnan(out[4][[0, 2]]).all()
    for k in ref:
        assert np.array_equal(got[k][1], ref[k]), k
    for k in before:
        assert np.array_equal(got[k][[0, 2]], before[k][[0, 2]]), k
    # ... their filters' host rows too: a later update of everybody starts, for them, from the first observation and step count
    fresh_sb, fresh_mb = _setup(case, envs)
    a_next = np.where(np.isnan(out[1][-1]), np.float32(0.25), out[1][-1])
    x_next = np.where(np.isnan(out[0][-1]), st + np.float32(0.01), out[0][-1])
    mb.optimize(a_next, x_next, case["mpf_bw"], case["mpf_steps"])
    fresh_mb.optimize(a_next, x_next, case["mpf_bw"], case["mpf_steps"])
    assert np.array_equal(mb.get_particles()[[0, 2]], fresh_mb.get_particles()[[0, 2]])
    for h in (sb, mb, fresh_sb, fresh_mb):
        h.close()


# ------------------------------------------------------------------------------------------------ 5. launches and refusals
def _filter_launches(case, envs):
    st, ap, rows, seeds = _inputs(case, envs)
    sb, mb = _setup(case, envs)
    s0 = mb.stats()
    _episode(case, sb, mb, st, ap, rows, seeds, case["T"])
    s1 = mb.stats()
    sb.close()
    mb.close()
    return s1["launches"] - s0["launches"]


def test_launch_counts():
    case = cases.BY_ID["pend_sgd_silverman"]
    T = case["T"]
    st, ap, rows, seeds = _inputs(case)
    sb, mb = _setup(case)
    sb.ctx.profile(True)
    count = lambda: sb.ctx.profile_get().get("svmpc_batch_kernel", (0.0, 0))[1]
    total = lambda: sum(v[1] for v in sb.ctx.profile_get().values())
    _episode(case, sb, mb, st, ap, rows, seeds, 1)
    assert count() == 1 == total()
    _episode(case, sb, mb, st, ap, rows, seeds, T)
    assert count() == 1 + T == total()
    sb.close()
    mb.close()
    # the filter side: Silverman's rule and the update per period that has one, whatever B
    assert _filter_launches(case, [0]) == _filter_launches(case, [0, 1, 2, 1, 0]) == 2 * (T - 1)


def test_refusals_come_before_anything_is_staged_or_launched():
    L = _L()
    case = cases.BY_ID["pend_sgd_silverman"]
    B, T, n = case["B"], case["T"], case["n_steps"]
    st, _, rows, seeds = _inputs(case)
    sb, mb = _setup(case)
    out = _episode(case, sb, mb, st, None, rows, seeds, 2)  # (so that every getter has something to keep)
    ap = out[1][-1]
    sb.ctx.profile(True)
    total = lambda: sum(v[1] for v in sb.ctx.profile_get().values())
    before, stats = _state(sb, mb), mb.stats()
    lib, FP = L.load(), L.FP
    f = lambda a: np.ascontiguousarray(a, np.float32)
    sp, app, lp, sd = f(out[0][-1]), f(ap), f(rows), np.ascontiguousarray(seeds[:T])
    xs, ac, pw, bw, sq = (np.zeros(s, np.float32) for s in ((T, B, 2), (T, B, 1), (T, B, case["N"]), (T, B), (B, case["H"], 1)))
    P = lambda a: None if a is None else a.ctypes.data_as(FP)
    S = lambda a: None if a is None else a.ctypes.data_as(L.C.POINTER(L.C.c_uint64))

    def call(sbh=sb._h, mbh=mb._h, states=sp, prev=app, periods=T, n_steps=n, mpf_steps=case["mpf_steps"], sds=sd, plt=lp, flags=0, so=xs, ao=ac):
        return lib.dust_svmpc_dual_batch_episode(sbh, mbh, P(states), P(prev), periods, n_steps, mpf_steps, -1.0, S(sds), P(plt), flags, None,
                                                 P(so), P(ao), P(pw), P(bw), P(sq))

    other_sb, other_mb = _setup(case, [0, 1])  # another n_env: no pair
    refused = [(call(states=None), L.ERR_INVALID), (call(so=None), L.ERR_INVALID), (call(ao=None), L.ERR_INVALID), (call(sds=None), L.ERR_INVALID),
               (call(periods=0), L.ERR_INVALID), (call(periods=4097), L.ERR_INVALID), (call(n_steps=0), L.ERR_INVALID),
               (call(mpf_steps=-1), L.ERR_INVALID), (call(mpf_steps=4097), L.ERR_INVALID), (call(mbh=other_mb._h), L.ERR_INVALID),
               (call(sbh=None), L.ERR_INVALID), (call(mbh=None), L.ERR_INVALID),
               (call(flags=L.SVMPC_BATCH_KEEP_ACTIONS), L.ERR_UNSUPPORTED), (call(flags=L.PTR_DEVICE), L.ERR_UNSUPPORTED),
               (call(flags=L.STORE_STATES), L.ERR_UNSUPPORTED)]
    for k, (got, want) in enumerate(refused):
        assert got == want, (k, got, want)
    assert total() == 0 and mb.stats() == stats
    _same(_state(sb, mb), before)
    assert not xs.any() and not ac.any() and not pw.any() and not bw.any() and not sq.any()  # nothing was written either
    # ... and the filters' host rows stand: the same further tick as on a pair that was never refused anything
    sb2, mb2 = _setup(case)
    _episode(case, sb2, mb2, st, None, rows, seeds, 2)
    for u, v in zip(_tick(case, sb, mb, out[0][-1], ap, seeds[2]), _tick(case, sb2, mb2, out[0][-1], ap, seeds[2])):
        assert np.array_equal(u, v)
    _same(_state(sb, mb), _state(sb2, mb2))
    for h in (sb, mb, sb2, mb2, other_sb, other_mb):
        h.close()


def test_plant_rows_without_uncertain_parameters_are_refused():
    """dim_p = 0 has no columns a true row could fill (and no filter to pair with: the refusal comes first)"""
    from dust_amd import Context

    L = _L()
    case = ec.BY_ID["one"]
    c = Context(**ec.context_kwargs(case))
    sb = c.svmpc_batch(1, seeds=[1])
    c.close()
    dual = cases.BY_ID["ones"]
    sb1, mb1 = _setup(dual)
    sb.ctx.profile(True)
    with pytest.raises(L.DustError) as e:
        sb.dual_episode(mb1, np.zeros((1, 2), np.float32), 1, 1, seeds=np.ones((1, 1), np.uint64), plant_params=np.ones((1, 1), np.float32))
    assert e.value.status == L.ERR_INVALID and sum(v[1] for v in sb.ctx.profile_get().values()) == 0
    for h in (sb, sb1, mb1):
        h.close()


@pytest.mark.parametrize("family,up", [("cartpole", ("mass_pole", "length")), ("skid_steer", ("x_icr", "wheel_radius"))])
def test_host_likelihood_pairs_are_unsupported(family, up):
    from test_gpu_svmpc_dual_batch import _setup as pair

    L = _L()
    B, T = 2, 2
    sb, mb, states, _ = pair(family, up, False, 3, 8, 2, 4, 16, "SGD", "K1", B, [5, 6])
    sb.ctx.profile(True)
    x0, stats = mb.get_particles(), mb.stats()
    th0 = sb.get(L.SVB_THETA)
    with pytest.raises(L.DustError) as e:
        sb.dual_episode(mb, states, T, 1, mpf_steps=2, mpf_bw=0.05, seeds=np.arange(1, T * B + 1, dtype=np.uint64).reshape(T, B))
    assert e.value.status == L.ERR_UNSUPPORTED
    assert sum(v[1] for v in sb.ctx.profile_get().values()) == 0 and mb.stats() == stats
    assert np.array_equal(mb.get_particles(), x0) and np.array_equal(sb.get(L.SVB_THETA), th0)
    # the pair still ticks period by period
    a_seq, _, _, _ = sb.dual_tick(mb, states, None, n_steps=1, mpf_steps=2, mpf_bw=0.05, seeds=[1, 2])
    assert np.isfinite(a_seq).all()
    sb.close()
    mb.close()


# ------------------------------------------------------------------------------------------------ 6. the class
def _example(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "examples", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _loop(B=3):
    """the example's scenario at test size: B pendulums with their own true (length, mass)"""
    loop, _, start, (length, mass) = _example("svmpc_dual_batch_example").scenario(B, 3, 16, 3, 6, 16, seed=3, mpf_steps=3)
    return loop, start, torch.stack((length, mass), 1)


def test_run_episodes_against_ticks_of_the_class():
    B, T = 3, 3
    ep, st0, true = _loop(B)
    a0, _ = ep.forward(st0)  # (creates the device batches, so that the deep copy below carries them; period 1 of the loop)
    x1 = st0 + 0.01
    ep.step(a0[:, 0], x1)  # a noted update: period 0 of the episode folds it in
    ticks = copy.deepcopy(ep)
    xs, acts, pw, a_seq = ep.run_episodes(x1, T, plant_params=true)
    assert all(isinstance(v, torch.Tensor) for v in (xs, acts, pw, a_seq)) and tuple(xs.shape) == (T, B, 2) and tuple(acts.shape) == (T, B, 1)
    replay = iter(xs)
    x = x1
    for t in range(T):
        a_t, x, pw_t = ticks.tick(x, lambda states, actions: next(replay))
        assert torch.equal(a_t, acts[t]) and torch.equal(pw_t, pw[t]) and torch.equal(x, xs[t]), t
    assert ep._t == ticks._t == 1 + T and ep.ticks == ticks.ticks == 1 + T
    assert torch.equal(ep.theta, ticks.theta)
    for u, v in zip(ep._pending, ticks._pending):
        assert np.array_equal(u, v)
    assert torch.equal(ep.last_bw, ticks.last_bw)
    both = copy.deepcopy(ep), copy.deepcopy(ticks)  # (dyn_particles folds the pending pair in: on copies, the loops go on below)
    assert torch.equal(both[0].dyn_particles, both[1].dyn_particles) and torch.equal(both[0].last_bw, both[1].last_bw)
    # a forward() after run_episodes against the copy's next forward()
    f1, f2 = ep.forward(xs[-1]), ticks.forward(xs[-1])
    assert torch.equal(f1[0], f2[0]) and torch.equal(f1[1], f2[1]) and torch.equal(ep.dyn_particles, ticks.dyn_particles)


def test_run_episodes_twice_against_once_and_a_deep_copy_between():
    B = 3
    once, st0, true = _loop(B)
    once.forward(st0)  # (creates the device batches, so that the deep copies below carry them)
    twice = copy.deepcopy(once)
    xs, acts, pw, a_seq = once.run_episodes(st0, 5, plant_params=true)
    x1, a1, w1, _ = twice.run_episodes(st0, 2, plant_params=true)
    twin = copy.deepcopy(twice)  # between two run_episodes calls: the pending pair travels
    assert twin._mb is not twice._mb and twin.svmpc._batch is not twice.svmpc._batch and twin._pending is not twice._pending
    for loop in (twice, twin):
        x2, a2, w2, s2 = loop.run_episodes(x1[-1], 3, plant_params=true, active=None)
        assert torch.equal(torch.cat((x1, x2)), xs) and torch.equal(torch.cat((a1, a2)), acts) and torch.equal(torch.cat((w1, w2)), pw)
        assert torch.equal(s2, a_seq) and torch.equal(loop.theta, once.theta) and loop._t == once._t == 6
        assert torch.equal(copy.deepcopy(loop).dyn_particles, copy.deepcopy(once).dyn_particles)
    # inactive environments: NaN rows, in both
    one = twice.run_episodes(xs[-1], 2, plant_params=true, active=[1, 0, 1])
    two = twin.run_episodes(xs[-1], 2, plant_params=true, active=[1, 0, 1])
    for u, v in zip(one, two):
        assert torch.equal(torch.nan_to_num(u, nan=7.0), torch.nan_to_num(v, nan=7.0))
    assert bool(torch.isnan(one[0][:, 1]).all()) and bool(torch.isnan(one[1][:, 1]).all())


def test_a_refused_call_keeps_the_keys_and_the_noted_update():
    L = _L()
    loop, st0, true = _loop(2)
    a, _ = loop.forward(st0)
    loop.step(a[:, 0], st0 + 0.01)
    t, pend, ticks = loop._t, loop._pending, loop.ticks
    loop.mpf_steps = -1  # (the library refuses a negative step count)
    with pytest.raises(L.DustError):
        loop.run_episodes(st0 + 0.01, 2, plant_params=true)
    with pytest.raises(ValueError):
        loop.run_episodes(st0 + 0.01, 0, plant_params=true)
    assert loop._t == t and loop._pending is pend and pend is not None and loop.ticks == ticks
    loop.mpf_steps = 3
    xs, acts, _, _ = loop.run_episodes(st0 + 0.01, 2, plant_params=true)
    assert torch.isfinite(xs).all() and loop._t == t + 2 and loop.ticks == ticks + 2
    assert np.array_equal(loop._pending[0], acts[-1].numpy()) and np.array_equal(loop._pending[1], xs[-1].numpy())


# ------------------------------------------------------------------------------------------------ 7. the example
def test_the_example_runs_tiny():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "svmpc_dual_episode_example.py"), "--tiny"], capture_output=True, text=True,
                         timeout=300, env=dict(os.environ, PYTHONPATH=ROOT))
    assert out.returncode == 0, out.stderr[-2000:]
    costs = [float(line.split("average cost")[1].split()[0]) for line in out.stdout.splitlines() if "average cost" in line]
    assert len(costs) == 3 and np.isfinite(costs).all(), out.stdout
