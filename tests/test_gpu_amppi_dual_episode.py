"""Dual AMPPI episodes on the device (dust_amppi_dual_batch_episode, `AmppiBatch.dual_episode`, `BatchDualAMPPI.run_episodes`;
csrc/amppi_episode.hpp amppi_prior_period_kernel / amppi_period_kernel): T periods of filter update, tick, plant step, roll and the
conditioning of the filters' rows, chained on one stream.  Every np.array_equal below is bit for bit.

An episode against T `dust_amppi_dual_batch_tick` calls on clones of both batches fed the episode's recorded states and actions: costs,
omega, first actions, bandwidths, the last sequence, and afterwards the sequences, the stored actions, the filters' particles, prior
bandwidths and `dust_mpf_batch_stats`; the optimiser slots, step counts and the filters' host rows show through one further dual tick on
both.  In the extended, single and sigma modes, Mp = 1 / 3 / 65, Silverman and fixed bandwidths, with and without `actions_prev`; chained
episodes; inactive neighbours; a launch count independent of B; the skid-steer / cart-pole refusal ahead of any staging.  The plant's
arithmetic is held to float64 by tests/test_gpu_amppi_episode.py (the same tail of the same kernel family)."""
import numpy as np
import pytest

from test_gpu_amppi_dual import MPF_STEPS
from test_gpu_amppi_dual_batch import B, SEEDS, _batch_pair

pytestmark = pytest.mark.gpu

T = 3
SCALE = [None]  # the sigma scale of the last _setup, or None
REL = np.array([1.25, 0.8, 1.15], np.float32)  # the true rows: the filters' mean particle, 15 - 25 % off per environment


@pytest.fixture(autouse=True)
def _single_workgroup_filters(monkeypatch):
    monkeypatch.setenv("DUST_MPF_GRID", "0")


def _setup(family, mode, S, H, Mp, optimizer="SGD"):
    pairs, batch, mb, states, _ = _batch_pair(family, mode, S, H, Mp, optimizer=optimizer)
    for c, m, _, _ in pairs:
        c.close()
        m.close()
    SCALE[0] = pairs[0][3]
    plant = (mb.get_particles().mean(1) * REL[:B, None]).astype(np.float32)
    return batch, mb, states, plant


def _keys(base, n=T):
    return np.array([[base + t + (b << 32) for b in range(B)] for t in range(n)], np.uint64)


def _ticks(tb, tm, states, prev, xs, acts, keys, mode, bw, active=None):
    """the episode's periods as dual ticks on the clones, fed the recorded states and actions -> [(costs, omega, a_seq, bw_used)]"""
    out, x = [], states
    for t in range(len(keys)):
        costs, omega, aseq, _, bwu = tb.dual_tick(tm, x, prev, None, shared_params=mode == "single", mpf_steps=MPF_STEPS, mpf_bw=bw,
                                                  seeds=keys[t], roll=1, active=active)
        out.append((costs, omega, aseq, bwu))
        on = np.ones(B, bool) if active is None else np.asarray(active, bool)
        prev = np.where(on[:, None], acts[t], 0.0 if prev is None else prev).astype(np.float32)
        x = np.where(on[:, None], xs[t], x).astype(np.float32)
    return out


def _state_of(batch, mb):
    return dict(a_seq=batch.get_a_seq(), acts=batch.get_actions(), x=mb.get_particles(), pbw=mb.get_prior_bw())


def _same_state(u, v):
    for k in u:
        assert np.array_equal(u[k], v[k], equal_nan=True), k


def _plant_check(states, xs, acts, plant):
    """the plant stepped under the TRUE rows it was handed: every recorded state against the float64 step of tests/amppi_cases.py on the
    device's own previous state and action, within the tolerance measured from the restatement alone, and at least POWER tolerances from
    the nominal rows, the previous action and no step in at least one period (the method of tests/test_gpu_amppi_episode.py)"""
    import amppi_episode_cases as ec
    from helpers import elemerr

    case = ec.DUAL_PLANT
    tol = ec.plant_tolerance(case)
    prev = np.concatenate((states[None], xs[:-1]))
    ref = np.stack([ec.plant_step(case, prev[t], acts[t], plant) for t in range(len(xs))])
    err = elemerr(xs, ref)
    far = ec.distances(case, xs, prev, acts, plant, None, tol)
    print("dual plant err %.2e tol %.2e  " % (err, tol) + "  ".join("%s %.0f" % kv for kv in sorted(far.items())))
    assert err < tol, (err, tol)
    assert set(far) == {"nominal", "prev_action", "unstepped"}
    for k, v in far.items():
        assert v >= ec.POWER, (k, v)


CASES = [("pendulum", "extended", 257, 12, 65, None, False), ("pendulum", "extended", 1, 12, 1, 0.05, True),
         ("pendulum", "single", 255, 8, 3, None, True), ("pendulum", "sigma", 256, 8, 3, 0.05, False),
         ("particle", "extended", 65, 10, 3, None, True), ("particle", "sigma", 64, 10, 65, None, False)]


@pytest.mark.parametrize("family,mode,S,H,Mp,bw,first", CASES, ids=["-".join(str(v) for v in c) for c in CASES])
def test_dual_episode_equals_its_dual_ticks(family, mode, S, H, Mp, bw, first):
    batch, mb, states, plant = _setup(family, mode, S, H, Mp, optimizer="Adam" if Mp == 3 else "SGD")
    tb, tm = batch.clone(), mb.clone()
    if SCALE[0] is not None:  # (the transform's scale is the context's: a clone is handed it as the batch was)
        tb.ctx.set_sigma_scale(SCALE[0])
    prev0 = (0.2 * np.arange(1, B * batch.da + 1, dtype=np.float32)).reshape(B, batch.da) if first else None
    keys = _keys(900)
    s0 = mb.stats()
    xs, acts, costs, omega, bwu, a_seq = batch.dual_episode(mb, states, T, prev0, shared_params=mode == "single", mpf_steps=MPF_STEPS, mpf_bw=bw,
                                                            seeds=keys, roll_steps=1, plant_params=plant)
    s1, t0 = mb.stats(), tm.stats()
    for v in (xs, acts, costs, omega, bwu, a_seq):
        assert np.isfinite(v).all()
    ticks = _ticks(tb, tm, states, prev0, xs, acts, keys, mode, bw)
    t1 = tm.stats()
    for t, (c_t, o_t, s_t, b_t) in enumerate(ticks):
        assert np.array_equal(c_t, costs[t]) and np.array_equal(o_t, omega[t]), t
        assert np.array_equal(s_t[:, 0], acts[t]) and np.array_equal(b_t, bwu[t]), (t, b_t, bwu[t])
    assert np.array_equal(ticks[-1][2], a_seq)
    _same_state(_state_of(batch, mb), _state_of(tb, tm))
    assert {k: s1[k] - s0[k] for k in s0} == {k: t1[k] - t0[k] for k in t0}, (s0, s1, t0, t1)
    assert not np.array_equal(xs[0], xs[1]) and not np.array_equal(costs[0], costs[1])
    if family == "pendulum" and mode == "extended" and S == 257:
        _plant_check(states, xs, acts, plant)
    # one further dual tick on both: the pending pair, the filters' host rows, optimiser slots and step counts, the stream positions
    k2 = _keys(950, 1)[0]
    one = batch.dual_tick(mb, xs[-1], acts[-1], None, shared_params=mode == "single", mpf_steps=MPF_STEPS, mpf_bw=bw, seeds=k2, roll=1)
    two = tb.dual_tick(tm, xs[-1], acts[-1], None, shared_params=mode == "single", mpf_steps=MPF_STEPS, mpf_bw=bw, seeds=k2, roll=1)
    for u, v in zip(one, two):
        assert (u is None and v is None) or np.array_equal(u, v)
    _same_state(_state_of(batch, mb), _state_of(tb, tm))
    for o in (batch, mb, tb, tm):
        o.close()


def test_chained_dual_episodes_and_inactive_neighbours():
    """episode(1) then episode(T - 1) with the pending pair handed on is episode(T); under the mask (1, 0, 1) the middle environment
    keeps its sequence, particles and bandwidths, its rows are not written, and the others equal the masked dual ticks"""
    family, mode, S, H, Mp = "pendulum", "extended", 257, 12, 65
    batch, mb, states, plant = _setup(family, mode, S, H, Mp)
    cb, cm = batch.clone(), mb.clone()
    keys = _keys(700)
    kw = dict(mpf_steps=MPF_STEPS, roll_steps=1, plant_params=plant)
    whole = batch.dual_episode(mb, states, T, None, seeds=keys, **kw)
    a = cb.dual_episode(cm, states, 1, None, seeds=keys[:1], **kw)
    b = cb.dual_episode(cm, a[0][-1], T - 1, a[1][-1], seeds=keys[1:], **kw)
    for k in range(5):
        assert np.array_equal(np.concatenate((a[k], b[k])), whole[k]), k
    assert np.array_equal(b[5], whole[5])
    _same_state(_state_of(batch, mb), _state_of(cb, cm))
    # the mask, continuing both
    tb, tm = batch.clone(), mb.clone()
    before = _state_of(batch, mb)
    on = np.array([1, 0, 1], np.uint8)
    keys = _keys(800)
    xs, acts, costs, omega, bwu, a_seq = batch.dual_episode(mb, whole[0][-1], T, whole[1][-1], seeds=keys, active=on, **kw)
    ticks = _ticks(tb, tm, whole[0][-1], whole[1][-1], xs, acts, keys, mode, None, active=on)
    for t, (c_t, o_t, s_t, b_t) in enumerate(ticks):
        for e in (0, 2):
            assert np.array_equal(c_t[e], costs[t][e]) and np.array_equal(o_t[e], omega[t][e]) and np.array_equal(s_t[e, 0], acts[t][e]), (t, e)
            assert b_t[e] == bwu[t][e], (t, e)
    for v in (xs, acts, costs, omega, bwu):
        assert np.isnan(v[:, 1]).all() and np.isfinite(v[:, [0, 2]]).all()
    assert np.isnan(a_seq[1]).all()
    after = _state_of(batch, mb)
    for k in ("a_seq", "x", "pbw"):
        assert np.array_equal(after[k][1], before[k][1]), k
    _same_state(after, _state_of(tb, tm))
    for o in (batch, mb, cb, cm, tb, tm):
        o.close()


def _counts(nb):
    """profile and stats counters added by one episode of T periods with an update in each, extended mode, Silverman bandwidths"""
    from dust_amd import Context, MpfContext

    c = Context(model="pendulum", N=1, S=257, M=1, H=12, temperature=100.0, alpha=0.01, sigma_a=2.0, uncertain_params=("length", "mass"), seed=3)
    rng = np.random.default_rng(1)
    m = MpfContext((1.0 + 0.05 * rng.standard_normal((48, 2))).astype(np.float32), np.array([3.0, 0.0], np.float32), model="pendulum",
                   uncertain_params=("length", "mass"), obs_std=0.2, lr=1e-6, init_bw=0.05)
    batch, mb = c.amppi_batch(nb), m.batch(nb)
    states = np.tile(np.array([3.0, 0.0], np.float32), (nb, 1))
    mb.set_obs(states)
    keys = np.array([[1 + t + (b << 32) for b in range(nb)] for t in range(T)], np.uint64)
    batch.ctx.profile(True)
    s0 = mb.stats()
    out = batch.dual_episode(mb, states + 0.01, T, np.zeros((nb, 1), np.float32), seeds=keys, mpf_steps=MPF_STEPS)
    prof, s1 = batch.ctx.profile_get(), mb.stats()
    assert all(np.isfinite(v).all() for v in out)
    for o in (batch, mb, c, m):
        o.close()
    return {k: v[1] for k, v in prof.items()}, {k: s1[k] - s0[k] for k in s0}


def test_launch_count_does_not_depend_on_B():
    p1, s1 = _counts(1)
    p5, s5 = _counts(5)
    assert p1 == p5 and s1 == s5, (p1, p5, s1, s5)
    assert p1 == {"amppi_kernel": T}, p1  # one period kernel per period, no roll launch
    assert s1 == dict(launches=2 * T, calls=T), s1  # (Silverman's rule and the update, per period)


def test_a_skid_steer_pair_is_refused_ahead_of_any_staging():
    from dust_amd import _lib as L

    for family in ("skid", "cartpole"):
        batch, mb, states, plant = _setup(family, "extended", 64, 8, 3)
        batch.ctx.profile(True)
        before, s0 = _state_of_pair(batch, mb), mb.stats()
        with pytest.raises(L.DustError, match="Pendulum and Particle pairs") as e:
            batch.dual_episode(mb, states, 2, None, seeds=_keys(1, 2), plant_params=plant)
        assert e.value.status == L.ERR_UNSUPPORTED
        assert batch.ctx.profile_get() == {} and mb.stats() == s0
        after = _state_of_pair(batch, mb)
        for k in before:
            assert np.array_equal(before[k], after[k]), k
        batch.close()
        mb.close()


def _state_of_pair(batch, mb):
    return dict(a_seq=batch.get_a_seq(), x=mb.get_particles(), pbw=mb.get_prior_bw())


def test_refusals_keep_the_getters():
    from dust_amd import _lib as L

    batch, mb, states, plant = _setup("pendulum", "extended", 64, 8, 3)
    batch.ctx.profile(True)
    before, s0 = _state_of_pair(batch, mb), mb.stats()
    lib, FP = L.load(), L.FP
    P = lambda a: None if a is None else a.ctypes.data_as(FP)
    keys = np.ascontiguousarray(_keys(1, 2).reshape(-1))
    KP = keys.ctypes.data_as(__import__("ctypes").POINTER(__import__("ctypes").c_uint64))
    xs, ac = np.zeros((2, B, 2), np.float32), np.zeros((2, B, 1), np.float32)

    def call(st=states, T=2, flags=0, steps=MPF_STEPS, roll=1, kp=KP, so=xs, ao=ac):
        return lib.dust_amppi_dual_batch_episode(batch._h, mb._h, P(st), None, T, flags, steps, -1.0, kp, roll, P(plant), None, P(so), P(ao), None, None,
                                                 None, None)

    refused = [(call(st=None), L.ERR_INVALID), (call(so=None), L.ERR_INVALID), (call(ao=None), L.ERR_INVALID), (call(kp=None), L.ERR_INVALID),
               (call(T=0), L.ERR_INVALID), (call(T=4097), L.ERR_INVALID), (call(roll=0), L.ERR_INVALID), (call(steps=-1), L.ERR_INVALID),
               (call(flags=L.PTR_DEVICE), L.ERR_UNSUPPORTED), (call(flags=L.STORE_STATES), L.ERR_UNSUPPORTED), (call(flags=L.STORE_F16), L.ERR_UNSUPPORTED)]
    for got, want in refused:
        assert got == want, (got, want)
    assert batch.ctx.profile_get() == {} and mb.stats() == s0 and not xs.any() and not ac.any()
    after = _state_of_pair(batch, mb)
    for k in before:
        assert np.array_equal(before[k], after[k]), k
    batch.close()
    mb.close()


def test_run_episodes_of_the_class_against_its_ticks():
    """BatchDualAMPPI.run_episodes(T) on the example's scenario against forward() / step() of a deep copy fed the recorded states and
    actions, bit for bit - costs, weights, first actions, sequences, particles - and then again from the pair it leaves pending"""
    import copy

    import torch

    from test_gpu_amppi_dual_batch import _example

    ex = _example()
    loop, plant, start, _ = ex.scenario(n_envs=B, samples=256, horizon=12, mpf_particles=32, seed=2)
    actions, states, _ = loop.tick(start.clone(), plant)  # (creates both device batches, and leaves an update noted)
    true = torch.tensor([[1.2, 0.8], [0.8, 1.1], [1.0, 1.3]])[:, :loop.mpf._dev.P]
    for piece in range(2):
        twin = copy.deepcopy(loop)
        xs, acts, costs, omega = loop.run_episodes(states, T, plant_params=true)
        x = states
        for t in range(T):
            a_seq, w = twin.forward(x)
            assert torch.equal(a_seq[:, 0], acts[t]) and torch.equal(w, omega[t]) and torch.equal(twin.last_costs, costs[t]), (piece, t)
            twin.step(acts[t], xs[t])
            x = xs[t]
        assert torch.equal(loop.a_seq, twin.a_seq)
        assert loop._t == twin._t and loop.ticks == twin.ticks and torch.equal(loop.last_bw, twin.last_bw)
        assert np.array_equal(loop._pending[0], twin._pending[0]) and np.array_equal(loop._pending[1], twin._pending[1])
        states = xs[-1]
    assert torch.equal(loop.dyn_particles, twin.dyn_particles)  # (carries the pending update out on both)


def _slot_batches(base, envs):
    """the two batches whose slot k holds environment envs[k] of `base` (its seed, sequence, particles, first observation)"""
    c0, m0, a0, x0, st0 = base
    batch = c0.amppi_batch(len(envs), seeds=[SEEDS[e] for e in envs])
    batch.set_a_seq(a0[envs])
    mb = m0.batch(len(envs))
    mb.set_particles(x0[envs])
    mb.set_obs(st0[envs])
    return batch, mb


@pytest.mark.parametrize("mode,bw", [("extended", None), ("single", 0.05)])
def test_an_environment_does_not_depend_on_its_slot(mode, bw):
    """environment 1 with its own filter particles, state, plant row and key: alone, and in slots 0 / 2 / 4 of five, it computes the bits
    it computes in slot 1 of three - records, sequence, stored actions, particles, prior bandwidths - and again in a second episode on
    clones of both batches taken after the first (the pending pair handed on)"""
    family, S, H, Mp, e = "pendulum", 257, 12, 65, 1
    pairs, batch, mb, states, _ = _batch_pair(family, mode, S, H, Mp)
    base = (pairs[0][0], pairs[0][1], batch.get_a_seq(), mb.get_particles(), states)
    plant = (base[3].mean(1) * REL[:B, None]).astype(np.float32)
    keys = [_keys(600), _keys(650)]
    kw = dict(shared_params=mode == "single", mpf_steps=MPF_STEPS, mpf_bw=bw, roll_steps=1)

    def run(bt, mf, envs):
        """two chained episodes, the second on clones taken between them -> every record of both, and the state behind each"""
        envs = np.asarray(envs)
        k0, k1 = (np.ascontiguousarray(k[:, envs]) for k in keys)  # (an environment's key goes with it)
        one = bt.dual_episode(mf, states[envs], T, None, seeds=k0, plant_params=plant[envs], **kw)
        s1 = _state_of(bt, mf)
        cb, cm = bt.clone(), mf.clone()
        two = cb.dual_episode(cm, one[0][-1], T, one[1][-1], seeds=k1, plant_params=plant[envs], **kw)
        s2 = _state_of(cb, cm)
        for o in (cb, cm):
            o.close()
        return one, s1, two, s2

    want = run(batch, mb, [0, 1, 2])
    for o in (batch, mb):
        o.close()

    def check(got, slot):
        for w, g in ((want[0], got[0]), (want[2], got[2])):  # records [T, B, .] and the last sequence [B, H, da]
            for k in range(5):
                assert np.array_equal(g[k][:, slot], w[k][:, e]), (slot, k)
            assert np.array_equal(g[5][slot], w[5][e]), slot
        for w, g in ((want[1], got[1]), (want[3], got[3])):
            for k in w:
                assert np.array_equal(g[k][slot], w[k][e]), (slot, k)

    alone = _slot_batches(base, [e])
    check(run(*alone, [e]), 0)
    envs = [e, 0, e, 2, e]
    five = _slot_batches(base, envs)
    got = run(*five, envs)
    for slot in (0, 2, 4):
        check(got, slot)
    assert not np.array_equal(got[0][0][:, 0], got[0][0][:, 1])  # (the neighbours are other environments)
    for o in alone + five:
        o.close()
    for c, m, _, _ in pairs:
        c.close()
        m.close()


def test_staging_and_record_bounds_are_refused_ahead_of_any_read():
    """2^28 values of staged parameter rows, or of records, per call: beyond either the plain episode refuses with DUST_ERR_UNSUPPORTED and
    says to split the episode - before it reads the (here far too small) arrays or launches anything"""
    import ctypes as C

    import amppi_cases as ac
    from dust_amd import Context, _lib as L

    s = ac.A("bound", "pendulum", 65536, 1, "extended", ("length", "mass"), 5)
    c = Context(**ac.context_kwargs(s))
    batch = c.amppi_batch(1)
    c.close()
    batch.ctx.profile(True)
    lib, FP = L.load(), L.FP
    small = np.zeros(16, np.float32)
    P = small.ctypes.data_as(FP)
    before = batch.get_a_seq()
    # 4096 periods x 65536 rows x 2 columns = 2^29 values to stage
    assert lib.dust_amppi_batch_episode(batch._h, P, 4096, P, 0, 1, None, None, P, P, None, None, None) == L.ERR_UNSUPPORTED
    assert "split the episode" in lib.dust_last_error().decode()
    # 2048 periods: 2^28 values to stage pass the first bound (it is "more than"); costs and omega records are 2 x 2^27 + ... values
    assert lib.dust_amppi_batch_episode(batch._h, P, 2048, P, 0, 1, None, None, P, P, P, P, None) == L.ERR_UNSUPPORTED
    assert "split the episode" in lib.dust_last_error().decode() and "record" in lib.dust_last_error().decode()
    assert batch.ctx.profile_get() == {} and np.array_equal(batch.get_a_seq(), before) and not small.any()
    batch.close()
