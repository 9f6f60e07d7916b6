"""Dual AMPPI episodes under the reference's rules on the device (dust_amppi_dual_batch_simulate, `AmppiBatch.dual_simulate`,
`BatchDualAMPPI.simulate`, `run_particle_episodes(mpf=)`; csrc/amppi_episode.hpp amppi_prior_sim_period_kernel /
amppi_sim_period_kernel): T periods of filter update, tick, plant step, cost, crash and goal chained on one stream, a stopped environment
skipped on both sides.  Every np.array_equal below is bit for bit; the cases are tests/amppi_sim_cases.py `DUAL`.

A call against `dust_amppi_dual_batch_tick` per period on clones of both batches, fed the recorded states and actions, with the rules on
the host through the fp32 replicas and stopped environments deactivated: costs, omega, actions, bandwidths, n_run, status, the
sequences, the stored actions, the filters' particles, prior bandwidths and `dust_mpf_batch_stats`, and one further dual tick on both
with every environment's pending pair (the filters' host rows, optimiser slots and step counts show there).  Rules off against
dust_amppi_dual_batch_episode; two chained calls against one; the filter-side launch count; the refusals; the class and the driver.  The
loss is the sequential fp32 sum of the recorded costs; every cost and every state of the three cases is held to the float64 restatement
as in tests/test_gpu_amppi_sim.py.  An environment does not depend on its batch: alone, in slots 0 / 2 / 4 of five, beside inactive,
already-stopped, earlier- and later-stopping neighbours, and from clones taken between two calls."""
import copy

import numpy as np
import pytest
import torch

import amppi_sim_cases as cases
from test_gpu_amppi_dual import MPF_STEPS
from test_gpu_amppi_dual_batch import B
from test_gpu_amppi_dual_episode import SCALE, _keys, _same_state, _setup, _state_of

pytestmark = pytest.mark.gpu

NAMES = ("xs", "acts", "costs", "omega", "bw", "ic", "loss", "status", "n_run", "a_seq")


@pytest.fixture(autouse=True)
def _single_workgroup_filters(monkeypatch):
    monkeypatch.setenv("DUST_MPF_GRID", "0")


def _make(d):
    batch, mb, states, plant = _setup(d["family"], d["mode"], d["S"], d["H"], d["Mp"], optimizer="Adam" if d["Mp"] == 3 else "SGD")
    if d["start"] is not None:
        states = np.asarray(d["start"], np.float32)
        mb.set_obs(states)
    return batch, mb, states, plant


def _kw(d, rules=True):
    r = d["rules"]
    kw = dict(shared_params=d["mode"] == "single", mpf_steps=MPF_STEPS, mpf_bw=d["bw"], roll_steps=1)
    if rules:
        kw.update(goal=r["goal"], goal_radius=r["radius"], stop_on_crash=r["crash"])
    return kw


def _sim(batch, mb, d, states, prev, keys, plant, rules=True, **extra):
    return dict(zip(NAMES, batch.dual_simulate(mb, states, len(keys), prev, seeds=keys, plant_params=plant, **_kw(d, rules), **extra)))


def _pending(r, states, prev):
    """every environment's pending pair behind a call: (actions[n - 1], states[n - 1]), or what it came with"""
    x, a = np.array(states, np.float32), (np.zeros_like(r["acts"][0]) if prev is None else np.array(prev, np.float32))
    for e in range(len(x)):
        n = int(r["n_run"][e])
        if n > 0:
            x[e], a[e] = r["xs"][n - 1, e], r["acts"][n - 1, e]
    return x, a


def _float64_checks(did, case, grid, r, states, plant):
    """every recorded cost against the float64 restatement on the device's own state, held away from the wrong costs the case can show,
    and every state against the float64 plant step on the device's own previous state and action (the method of
    tests/test_gpu_amppi_sim.py, here on the dual entry's kernels: amppi_prior_sim_period_kernel in the extended mode)"""
    from helpers import elemerr

    tol, ptol = cases.cost_tolerance(case), cases.plant_tolerance(case)
    pgrid = grid if case["family"] == "particle" else None
    new, prev, got, ref_x = [], [], [], []
    for e in range(B):
        for t in range(int(r["n_run"][e])):
            p = states[e] if t == 0 else r["xs"][t - 1, e]
            prev.append(p)
            new.append(r["xs"][t, e])
            got.append(r["ic"][t, e])
            ref_x.append(cases.plant_step(case, p[None], r["acts"][t, e][None], plant[e:e + 1], pgrid)[0])
    new, prev, got = np.array(new, np.float64), np.array(prev, np.float64), np.array(got)
    ref = cases.costs64(case, new, grid)
    err, perr = elemerr(got, ref), elemerr(new, np.array(ref_x))
    wrong = cases.cost_variants(case, prev, new, grid)
    far = {k: cases.variant_distance(got, v, tol) for k, v in wrong.items()}
    print("%-10s cost err %.2e tol %.2e plant err %.2e tol %.2e  " % (did, err, tol, perr, ptol) + "  ".join("%s %.0f" % kv for kv in sorted(far.items())))
    assert err < tol, (did, err, tol)
    assert perr < ptol, (did, perr, ptol)
    for k, v in far.items():
        if cases.shows(case, k):
            assert v >= cases.COST_POWER, (did, k, v)


@pytest.mark.parametrize("did", [d["id"] for d in cases.DUAL])
def test_call_equals_its_dual_ticks(did):
    d = cases.DUAL_BY_ID[did]
    case, T = cases.dual_as_case(d), d["T"]
    grid = cases.grid_of(case)
    batch, mb, states, plant = _make(d)
    tb, tm = batch.clone(), mb.clone()
    if SCALE[0] is not None:
        tb.ctx.set_sigma_scale(SCALE[0])
    prev0 = (0.2 * np.arange(1, B * batch.da + 1, dtype=np.float32)).reshape(B, batch.da) if d["first"] else None
    keys = _keys(900, T)
    s0, t0 = mb.stats(), tm.stats()
    r = _sim(batch, mb, d, states, prev0, keys, plant)
    s1 = mb.stats()
    on, x, prev = np.ones(B, bool), states.copy(), (None if prev0 is None else prev0.copy())
    n_host, st_host, last_seq, last_acts = np.zeros(B, np.int32), np.zeros(B, np.int32), [None] * B, [None] * B
    for t in range(T):
        if not on.any():
            break
        c_t, o_t, s_t, _, b_t = tb.dual_tick(tm, x, prev, None, shared_params=d["mode"] == "single", mpf_steps=MPF_STEPS, mpf_bw=d["bw"], seeds=keys[t],
                                             roll=1, active=on.astype(np.uint8))
        drawn = tb.get_actions()
        if prev is None:
            prev = np.zeros((B, batch.da), np.float32)
        for e in np.nonzero(on)[0]:
            assert np.array_equal(c_t[e], r["costs"][t, e]) and np.array_equal(o_t[e], r["omega"][t, e]), (t, e)
            assert np.array_equal(s_t[e, 0], r["acts"][t, e]) and b_t[e] == r["bw"][t, e], (t, e, b_t[e], r["bw"][t, e])
            last_seq[e], last_acts[e] = s_t[e], drawn[e]
            x[e], prev[e] = r["xs"][t, e], r["acts"][t, e]
        stat = cases.apply_rules(case, x, grid)
        n_host[on] += 1
        stop = on & (stat != 0)
        st_host[stop] = stat[stop]
        on &= ~stop
    t1 = tm.stats()
    assert np.array_equal(r["n_run"], n_host) and np.array_equal(r["status"], st_host), (r["n_run"], n_host, r["status"], st_host)
    for e in range(B):
        n = int(r["n_run"][e])
        for k in ("xs", "acts", "costs", "omega", "bw", "ic"):
            assert np.isnan(r[k][n:, e]).all() and np.isfinite(r[k][:n, e]).all(), (k, e)
        assert np.array_equal(r["a_seq"][e], last_seq[e]) and np.array_equal(batch.get_actions()[e], last_acts[e]), e
        want = np.float32(np.inf) if r["status"][e] == 2 else cases.loss32(r["ic"][:, e], n)
        assert np.array_equal(r["loss"][e], want), e
    _float64_checks(did, case, grid, r, states, plant)
    want = cases.DUAL_EVENTS.get(did)
    if want is not None:
        for e in range(B):
            period, status = want.get(e, (T - 1, 0))
            assert (r["n_run"][e], r["status"][e]) == (period + 1, status), e
    a, b_ = _state_of(batch, mb), _state_of(tb, tm)
    for k in ("a_seq", "x", "pbw"):
        assert np.array_equal(a[k], b_[k]), k
    # the filter side: the same launches and calls as the ticks, whatever stopped
    assert {k: s1[k] - s0[k] for k in s0} == {k: t1[k] - t0[k] for k in t0}, (s0, s1, t0, t1)
    # one further dual tick on both with every environment's pending pair: host rows, optimiser slots, step counts, stream positions
    x, a = _pending(r, states, prev0)
    k2 = _keys(950, 1)[0]
    kw = dict(shared_params=d["mode"] == "single", mpf_steps=MPF_STEPS, mpf_bw=d["bw"], seeds=k2, roll=1)
    one, two = batch.dual_tick(mb, x, a, None, **kw), tb.dual_tick(tm, x, a, None, **kw)
    for u, v in zip(one, two):
        assert (u is None and v is None) or np.array_equal(u, v)
    _same_state(_state_of(batch, mb), _state_of(tb, tm))
    for o in (batch, mb, tb, tm):
        o.close()


@pytest.mark.parametrize("did", ["pend_ext", "pend_sigma"])
def test_rules_off_is_the_dual_episode(did):
    d = cases.DUAL_BY_ID[did]
    batch, mb, states, plant = _make(d)
    cb, cm = batch.clone(), mb.clone()
    if SCALE[0] is not None:
        cb.ctx.set_sigma_scale(SCALE[0])
    keys = _keys(700, d["T"])
    r = _sim(batch, mb, d, states, None, keys, plant, rules=False)
    xs, acts, costs, omega, bw, a_seq = cb.dual_episode(cm, states, d["T"], None, shared_params=d["mode"] == "single", mpf_steps=MPF_STEPS,
                                                        mpf_bw=d["bw"], seeds=keys, roll_steps=1, plant_params=plant)
    for u, v in ((r["xs"], xs), (r["acts"], acts), (r["costs"], costs), (r["omega"], omega), (r["bw"], bw), (r["a_seq"], a_seq)):
        assert np.array_equal(u, v)
    assert (r["n_run"] == d["T"]).all() and not r["status"].any()
    _same_state(_state_of(batch, mb), _state_of(cb, cm))
    assert mb.stats() == cm.stats()
    for o in (batch, mb, cb, cm):
        o.close()


@pytest.mark.parametrize("cut", [1, 2])
def test_two_chained_calls_are_one(cut):
    """part_mass split behind environment 0's stop (period 0) and behind environment 2's (period 1)"""
    d = cases.DUAL_BY_ID["part_mass"]
    T = d["T"]
    batch, mb, states, plant = _make(d)
    cb, cm = batch.clone(), mb.clone()
    prev0 = np.full((B, batch.da), 0.3, np.float32)
    keys = _keys(800, T)
    whole = _sim(batch, mb, d, states, prev0, keys, plant)
    one = _sim(cb, cm, d, states, prev0, keys[:cut], plant)
    x, a = _pending(one, states, prev0)
    two = _sim(cb, cm, d, x, a, keys[cut:], plant, t0=cut, loss=one["loss"], status=one["status"])
    assert whole["n_run"].tolist() == [1, T, 2]
    for e in range(B):
        n1, n2 = int(one["n_run"][e]), int(two["n_run"][e])
        assert n1 + n2 == whole["n_run"][e], e
        for k in ("xs", "acts", "costs", "omega", "bw", "ic"):
            assert np.array_equal(np.concatenate((one[k][:n1, e], two[k][:n2, e])), whole[k][:n1 + n2, e]), (k, e)
    assert np.array_equal(two["loss"], whole["loss"]) and np.array_equal(two["status"], whole["status"])
    a, b_ = _state_of(batch, mb), _state_of(cb, cm)
    for k in ("a_seq", "x", "pbw"):  # (get_actions shows the environments of the LAST call: the second one's run mask)
        assert np.array_equal(a[k], b_[k]), k
    x, a = _pending(whole, states, prev0)  # one further dual tick on both: the filters' host rows, committed from n_run
    kw = dict(shared_params=True, mpf_steps=MPF_STEPS, mpf_bw=d["bw"], seeds=_keys(950, 1)[0], roll=1)
    for u, v in zip(batch.dual_tick(mb, x, a, None, **kw), cb.dual_tick(cm, x, a, None, **kw)):
        assert (u is None and v is None) or np.array_equal(u, v)
    _same_state(_state_of(batch, mb), _state_of(cb, cm))
    for o in (batch, mb, cb, cm):
        o.close()


@pytest.mark.parametrize("mode,bw", [("single", 0.05), ("extended", None)])
def test_an_environment_does_not_depend_on_its_batch(mode, bw):
    """environment 2 of part_mass (a crash in period 1) with its own filter particles, state, plant row and keys computes the same bits -
    records, loss, status, n_run, sequence, stored actions, filter particles, prior bandwidths, and one further dual tick - alone, in
    slots 0 / 2 / 4 of five beside an earlier-stopping and a never-stopping neighbour, beside an inactive and an already-stopped
    neighbour (which stay untouched on both sides), and from clones of both batches taken between two calls.  The filter-side counters
    do not depend on the batch either.  `single`: the staged rows and amppi_sim_period_kernel; `extended`: amppi_prior_sim_period_kernel
    and Silverman's rule"""
    from test_gpu_amppi_dual_batch import _batch_pair
    from test_gpu_amppi_dual_episode import REL, _slot_batches

    d = dict(cases.DUAL_BY_ID["part_mass"], mode=mode, bw=bw)
    T, e = d["T"], 2
    pairs, batch, mb, _, _ = _batch_pair(d["family"], mode, d["S"], d["H"], d["Mp"], optimizer="Adam")
    states = np.asarray(d["start"], np.float32)
    base = (pairs[0][0], pairs[0][1], batch.get_a_seq(), mb.get_particles(), states)
    for o in (batch, mb):
        o.close()
    plant = (base[3].mean(1) * REL[:B, None]).astype(np.float32)
    prev0 = (0.2 * np.arange(1, B * 2 + 1, dtype=np.float32)).reshape(B, 2)
    keys, k2 = _keys(600, T), _keys(650, 1)[0]

    def run(envs, **extra):
        """the call on a fresh pair of batches whose slot k holds environment envs[k], then one further dual tick of every slot with its
        pending pair -> (records, state behind the call, the further tick's outputs, the filters' counters the call added)"""
        envs = np.asarray(envs)
        bt, mf = _slot_batches(base, envs)
        before = dict(a_seq=bt.get_a_seq(), x=mf.get_particles(), pbw=mf.get_prior_bw())
        s0 = mf.stats()
        r = _sim(bt, mf, d, states[envs], prev0[envs], np.ascontiguousarray(keys[:, envs]), plant[envs], **extra)
        s1 = mf.stats()
        st = _state_of(bt, mf)
        x, a = _pending(r, states[envs], prev0[envs])
        more = bt.dual_tick(mf, x, a, None, shared_params=mode == "single", mpf_steps=MPF_STEPS, mpf_bw=bw, seeds=np.ascontiguousarray(k2[envs]), roll=1)
        st2 = _state_of(bt, mf)
        for o in (bt, mf):
            o.close()
        return r, st, more, st2, {k: s1[k] - s0[k] for k in s0}, before

    want = run([0, 1, 2])
    assert want[0]["n_run"].tolist() == [1, T, 2] and want[0]["status"].tolist() == [2, 0, 2]

    def check(got, slot):
        for k in ("xs", "acts", "costs", "omega", "bw", "ic"):
            assert np.array_equal(got[0][k][:, slot], want[0][k][:, e], equal_nan=True), (k, slot)
        for k in ("loss", "status", "n_run", "a_seq"):
            assert np.array_equal(got[0][k][slot], want[0][k][e]), (k, slot)
        for i in (1, 3):  # the state behind the call, and behind the further tick
            for k in want[i]:
                assert np.array_equal(got[i][k][slot], want[i][k][e]), (i, k, slot)
        for u, v in zip(got[2], want[2]):
            assert (u is None and v is None) or np.array_equal(u[slot], v[e]), slot
        assert got[4] == want[4], (got[4], want[4])  # the filter side's launches and calls: neither B nor the stops

    check(run([e]), 0)
    got = run([e, 0, e, 1, e])
    for slot in (0, 2, 4):
        check(got, slot)
    # slot 0 inactive, slot 1 already stopped (status 1 at entry), slot 3 stops earlier, slot 4 never
    loss0, stat0 = np.array([7.0, 5.0, 0.0, 0.0, 0.0], np.float32), np.array([0, 1, 0, 0, 0], np.int32)
    got = run([1, 1, e, 0, 1], active=[0, 1, 1, 1, 1], loss=loss0, status=stat0)
    check(got, 2)
    r = got[0]
    assert r["n_run"].tolist() == [-1, 0, 2, 1, T] and r["status"].tolist() == [0, 1, 2, 2, 0] and r["loss"][0] == 7.0 and r["loss"][1] == 5.0
    for k in ("xs", "acts", "costs", "omega", "bw", "ic"):
        assert np.isnan(r[k][:, :2]).all(), k
    assert np.isnan(r["a_seq"][:2]).all()
    for k in ("a_seq", "x", "pbw"):  # neither side of the two has moved
        assert np.array_equal(got[1][k][:2], got[5][k][:2]), k
    # clones of both batches between two calls finish as the originals do, and as the one call does
    bt, mf = _slot_batches(base, [0, 1, 2])
    one = _sim(bt, mf, d, states, prev0, keys[:1], plant)
    cb, cm = bt.clone(), mf.clone()
    x, a = _pending(one, states, prev0)
    two = [_sim(u, v, d, x, a, keys[1:], plant, t0=1, loss=one["loss"], status=one["status"]) for u, v in ((bt, mf), (cb, cm))]
    for k in NAMES:
        assert np.array_equal(two[0][k], two[1][k], equal_nan=True), k
    assert np.array_equal(two[0]["loss"], want[0]["loss"]) and np.array_equal(two[0]["status"], want[0]["status"])
    assert np.array_equal(two[0]["xs"][:1, e], want[0]["xs"][1:2, e])
    u, v = _state_of(bt, mf), _state_of(cb, cm)
    for k in ("a_seq", "x", "pbw"):
        assert np.array_equal(u[k], v[k]) and np.array_equal(u[k], want[1][k]), k
    for o in (bt, mf, cb, cm):
        o.close()
    for c, m, _, _ in pairs:
        c.close()
        m.close()


def _counts(nb, crash):
    """profile and stats counters added by one call of T = 3 periods, extended mode, Silverman bandwidths; crash: environment 0 (Particle,
    on an occupied cell) stops in period 0"""
    from dust_amd import Context, MpfContext
    from oracle import grid_4x4_map

    import amppi_cases as ac

    T = 3
    s = ac.A("counts", "particle", 65, 8, "extended", ("mass",), 3)
    c = Context(grid=grid_4x4_map(), seed=3, **ac.context_kwargs(s))
    rng = np.random.default_rng(1)
    st0 = np.array([-2.03, -6.04, 1.0, -2.0] if crash else [4.4, 0.3, -3.0, 4.5], np.float32)
    m = MpfContext((2.0 * (1.0 + 0.05 * rng.standard_normal((48, 1)))).astype(np.float32), st0, model="particle", uncertain_params=("mass",), obs_std=0.2,
                   lr=1e-6, init_bw=0.05, grid=grid_4x4_map(), mass=2.0)
    batch, mb = c.amppi_batch(nb), m.batch(nb)
    states = np.tile(st0, (nb, 1))
    mb.set_obs(states)
    keys = np.array([[1 + t + (b << 32) for b in range(nb)] for t in range(T)], np.uint64)
    batch.ctx.profile(True)
    s0 = mb.stats()
    out = batch.dual_simulate(mb, states, T, np.zeros((nb, 2), np.float32), seeds=keys, mpf_steps=MPF_STEPS, stop_on_crash=True)
    prof, s1 = batch.ctx.profile_get(), mb.stats()
    assert (out[8] == (1 if crash else T)).all()
    for o in (batch, mb, c, m):
        o.close()
    return {k: v[1] for k, v in prof.items()}, {k: s1[k] - s0[k] for k in s0}


def test_launch_counts_depend_neither_on_B_nor_on_the_stops():
    got = [_counts(nb, crash) for nb in (1, 5) for crash in (False, True)]
    for p, s in got:
        assert p == {"amppi_kernel": 3}, p  # one period kernel per period, no roll launch
        assert s == dict(launches=6, calls=3), s  # (Silverman's rule and the update, per period)


def test_refusals_keep_both_batches_and_the_in_out_arrays():
    import ctypes as C

    from dust_amd import _lib as L
    from dust_amd.backend import _episode_rules

    d = cases.DUAL_BY_ID["pend_ext"]
    batch, mb, states, plant = _make(d)
    batch.ctx.profile(True)
    before = dict(a_seq=batch.get_a_seq(), x=mb.get_particles(), pbw=mb.get_prior_bw())
    s0 = mb.stats()
    lib, FP, IP = L.load(), L.FP, C.POINTER(C.c_int)
    P = lambda a: None if a is None else a.ctypes.data_as(FP)
    PI = lambda a: None if a is None else a.ctypes.data_as(IP)
    keys = np.ascontiguousarray(_keys(1, 2).reshape(-1))
    KP = keys.ctypes.data_as(C.POINTER(C.c_uint64))
    SENT = np.float32(-77.0)
    xs, ac_, ic = np.full((2, B, 2), SENT, np.float32), np.full((2, B, 1), SENT, np.float32), np.full((2, B), SENT, np.float32)
    loss, status, n_run = np.full(B, 3.0, np.float32), np.zeros(B, np.int32), np.full(B, -5, np.int32)
    rules = lambda **kw: _episode_rules(2, kw.get("t0", 0), kw.get("warm_up", 0), (0.0, 0.0), kw.get("radius", 0.5), kw.get("crash", False))

    def call(st=states, T=2, flags=0, steps=MPF_STEPS, roll=1, kp=KP, so=xs, ao=ac_, ru=rules(), ico=ic, lo=loss, stt=status, nr=n_run):
        return lib.dust_amppi_dual_batch_simulate(batch._h, mb._h, P(st), None, T, flags, steps, -1.0, kp, roll, P(plant), None if ru is None else C.byref(ru),
                                                  None, P(so), P(ao), None, None, None, P(ico), P(lo), PI(stt), PI(nr), None)

    refused = [(call(st=None), L.ERR_INVALID), (call(so=None), L.ERR_INVALID), (call(ao=None), L.ERR_INVALID), (call(kp=None), L.ERR_INVALID),
               (call(T=0), L.ERR_INVALID), (call(T=4097), L.ERR_INVALID), (call(roll=0), L.ERR_INVALID), (call(steps=-1), L.ERR_INVALID),
               (call(ru=None), L.ERR_INVALID), (call(ico=None), L.ERR_INVALID), (call(lo=None), L.ERR_INVALID), (call(stt=None), L.ERR_INVALID),
               (call(nr=None), L.ERR_INVALID), (call(ru=rules(warm_up=2)), L.ERR_INVALID), (call(ru=rules(t0=-1)), L.ERR_INVALID),
               (call(ru=rules(radius=float("nan"))), L.ERR_INVALID), (call(stt=np.array([0, -1, 0], np.int32)), L.ERR_INVALID),
               (call(ru=rules(crash=True)), L.ERR_UNSUPPORTED),  # a Pendulum has no occupancy map
               (call(flags=L.PTR_DEVICE), L.ERR_UNSUPPORTED), (call(flags=L.STORE_STATES), L.ERR_UNSUPPORTED), (call(flags=L.STORE_F16), L.ERR_UNSUPPORTED)]
    for k, (got, want) in enumerate(refused):
        assert got == want, (k, got, want)
    assert batch.ctx.profile_get() == {} and mb.stats() == s0
    for v in (xs, ac_, ic):
        assert (v == SENT).all()
    assert (loss == 3.0).all() and not status.any() and (n_run == -5).all()
    after = dict(a_seq=batch.get_a_seq(), x=mb.get_particles(), pbw=mb.get_prior_bw())
    for k in before:
        assert np.array_equal(before[k], after[k]), k
    batch.close()
    mb.close()
    for family in ("skid", "cartpole"):
        batch, mb, states, plant = _setup(family, "extended", 64, 8, 3)
        batch.ctx.profile(True)
        s0 = mb.stats()
        with pytest.raises(L.DustError, match="Pendulum and Particle pairs") as e:
            batch.dual_simulate(mb, states, 2, None, seeds=_keys(1, 2), plant_params=plant)
        assert e.value.status == L.ERR_UNSUPPORTED and batch.ctx.profile_get() == {} and mb.stats() == s0
        batch.close()
        mb.close()


def test_the_record_cap_is_the_dual_episode_s():
    """more than 2^28 record values per call: DUST_ERR_UNSUPPORTED, before anything is read beyond the states, written or launched"""
    import ctypes as C

    import amppi_cases as ac
    from dust_amd import Context, MpfContext, _lib as L
    from dust_amd.backend import _episode_rules

    T = 2048  # costs and omega records: 2 x 2048 x 65536 = 2^28 values, and the states and actions on top
    s = ac.A("bound", "pendulum", 65536, 1, "extended", ("length", "mass"), 5)
    c = Context(**ac.context_kwargs(s))
    rng = np.random.default_rng(1)
    m = MpfContext((1.0 + 0.05 * rng.standard_normal((3, 2))).astype(np.float32), np.array([3.0, 0.0], np.float32), model="pendulum",
                   uncertain_params=("length", "mass"), obs_std=0.2, lr=1e-6, init_bw=0.05)
    batch, mb = c.amppi_batch(1), m.batch(1)
    batch.ctx.profile(True)
    lib, FP, IP = L.load(), L.FP, C.POINTER(C.c_int)
    small, loss, status, n_run = np.zeros(16, np.float32), np.full(1, 3.0, np.float32), np.zeros(1, np.int32), np.full(1, -5, np.int32)
    small[0] = 3.0
    P = small.ctypes.data_as(FP)
    keys = np.arange(1, T + 1, dtype=np.uint64)
    ru = _episode_rules(2, 0, 0, (0.0, 0.0), 0.5, False)
    before, s0 = (batch.get_a_seq(), mb.get_particles()), mb.stats()
    got = lib.dust_amppi_dual_batch_simulate(batch._h, mb._h, P, None, T, 0, MPF_STEPS, -1.0, keys.ctypes.data_as(C.POINTER(C.c_uint64)), 1, None,
                                             C.byref(ru), None, P, P, P, P, None, P, loss.ctypes.data_as(FP), status.ctypes.data_as(IP),
                                             n_run.ctypes.data_as(IP), None)
    assert got == L.ERR_UNSUPPORTED and "split the episode" in lib.dust_last_error().decode() and "record" in lib.dust_last_error().decode()
    assert batch.ctx.profile_get() == {} and mb.stats() == s0 and small[0] == 3.0 and not small[1:].any()
    assert np.array_equal(batch.get_a_seq(), before[0]) and np.array_equal(mb.get_particles(), before[1])
    assert loss[0] == 3.0 and status[0] == 0 and n_run[0] == -5
    for o in (batch, mb, c, m):
        o.close()


# ------------------------------------------------------------------------------------------------ the class and the driver
def _particle_loop(seed=5):
    """a Particle BatchAMPPI over the 4 x 4 grid, mass uncertain, and a filter prototype; the starts of `part_map`"""
    import amppi_cases as ac
    from dust_amd.controllers import BatchAMPPI
    from dust_amd.inference import MPF, GaussianLikelihood
    from dust_amd.models import Particle

    Bn, H, S = 4, 8, 64
    model = Particle(**ac.PART_ENV, mass=2.0, uncertain_params=("mass",))
    g = torch.Generator().manual_seed(seed)
    ctrl = BatchAMPPI(Bn, model.observation_space, model.action_space, H, S, lambda_=50.0, a_cov=25.0 * torch.eye(2),
                      inst_cost_fn=model.default_inst_cost, term_cost_fn=model.default_term_cost, params_sampling="extended",
                      init_actions=0.5 * torch.randn(H, 2, generator=g), seeds=[seed + b for b in range(Bn)])
    ctrl.return_rollouts = False
    start = torch.tensor(cases.BY_ID["part_map"]["start"])
    x0 = 2.0 * (1.0 + 0.05 * torch.randn(16, 1, generator=g))
    mpf = MPF(init_particles=x0, likelihood=GaussianLikelihood(initial_obs=start[0], obs_std=0.2, model=Particle(**ac.PART_ENV, mass=2.0, uncertain_params=("mass",)),
                                                             log_space=False), optimizer_class=torch.optim.SGD, lr=1e-3, bw=0.05, bw_scale=1.0)
    true = torch.tensor([[2.8], [1.4], [2.4], [1.7]])
    return ctrl, mpf, model, start, true


def test_the_class_against_its_ticks_and_resume_across_a_stop():
    """BatchDualAMPPI.simulate against forward() / step() of a deep copy with the rules on the host, and resume across the stops"""
    from dust_amd.controllers import BatchDualAMPPI

    case, grid = cases.BY_ID["part_map"], cases.grid_of(cases.BY_ID["part_map"])
    ctrl, mpf, model, start, true = _particle_loop()
    once = BatchDualAMPPI(ctrl, model, mpf, mpf_bw=0.5, mpf_steps=2, seed=11)
    once.model.params_dist = once.mpf.prior  # (creates both device batches, so that the deep copies below carry them)
    ctrl._ensure_batch(model)
    once._filters(start.numpy())
    ticks, pieces = copy.deepcopy(once), copy.deepcopy(once)
    kw = dict(goal=model.target, goal_radius=1.0, stop_on_crash=True, plant_params=true)
    T = 3
    full = once.simulate(start, T, **kw)
    assert full.status.tolist() == [2, 1, 2, 0] and full.n_run.tolist() == [1, 1, 2, 3] and bool(torch.isinf(full.loss[[0, 2]]).all())
    on, x = np.ones(4, bool), start.clone()
    for t in range(T):
        a_seq, w = ticks.forward(x, active=on.tolist())
        acts, new = torch.zeros(4, 2), x.clone()
        for e in np.nonzero(on)[0]:
            assert torch.equal(a_seq[e, 0], full.actions[t, e]) and torch.equal(w[e], full.omega[t, e]) and torch.equal(ticks.last_costs[e], full.costs[t, e]), (t, e)
            acts[e], new[e] = full.actions[t, e], full.states[t, e]
        stat = cases.apply_rules(case, new.numpy(), grid)
        x = new
        on &= stat == 0
        ticks.step(acts, new)
    assert torch.equal(once.a_seq, ticks.a_seq)
    first = pieces.simulate(start, 1, **kw)
    second = pieces.simulate(torch.nan_to_num(first.states[-1]), T - 1, resume=first, **kw)
    assert second.n_run.tolist() == [-1, -1, 1, 2] and second.t0 == T  # the stopped environments are passed as inactive
    assert torch.equal(second.loss[2:], full.loss[2:]) and torch.equal(first.loss[:2], full.loss[:2])
    assert torch.equal(pieces.a_seq, once.a_seq) and torch.equal(pieces.dyn_particles, once.dyn_particles)


def test_run_particle_episodes_with_a_filter_and_a_load_against_two_simulate_calls():
    from dust_amd.controllers import BatchDualAMPPI
    from dust_amd.utils.simulations import run_particle_episodes

    ctrl, mpf, model, start, true = _particle_loop()
    ctrl2 = copy.deepcopy(ctrl)
    steps, load = 8, 0.5
    loss = run_particle_episodes(start, model, None, ctrl, load=load, steps=steps, plant_params=true, mpf=mpf, mpf_bw=0.5, mpf_steps=2)
    dual = BatchDualAMPPI(ctrl2, model, mpf, mpf_bw=0.5, mpf_steps=2)
    kw = dict(goal=model.target, goal_radius=1.0, stop_on_crash=True)
    one = dual.simulate(start, steps // 4, plant_params=true, **kw)
    x = start.clone()
    for b in range(4):
        if one.n_run[b] > 0:
            x[b] = one.states[one.n_run[b] - 1, b]
    two = dual.simulate(x, steps - steps // 4, plant_params=true + load, resume=one, **kw)
    assert torch.equal(loss, two.loss) and bool(torch.isinf(loss[[0, 2]]).all()) and bool(torch.isfinite(loss[[1, 3]]).all())
    assert torch.equal(ctrl.a_seq, ctrl2.a_seq)
