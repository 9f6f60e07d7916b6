"""The dual loop over a batch of plants on the device: dust_mpf_batch_* (MpfContext.batch / MpfBatch), dust_amppi_dual_batch_tick
(AmppiBatch.dual_tick) and dust_amd.controllers.BatchDualAMPPI.  Every comparison is np.array_equal against the lone path - lone filters
created under DUST_MPF_GRID=0 (the switch is read once, in dust_mpf_create), so that they run the single-workgroup kernel whose arithmetic
the batch repeats; the lone path itself is pinned to the reference by tests/golden/amppi_dual_*.npz and the filter fixtures."""
import copy
import importlib.util
import os

import numpy as np
import pytest
import torch

from test_gpu_amppi_dual import MPF_STEPS, PIECES, UPS, _pair, _plant

pytestmark = pytest.mark.gpu

B = 3
SEEDS = (7, 11, 5)


@pytest.fixture(autouse=True)
def _single_workgroup_filters(monkeypatch):
    monkeypatch.setenv("DUST_MPF_GRID", "0")


def _env_plant(b, state, action):
    """a small host plant per environment (test_gpu_amppi_dual._plant with another gain): both sides see the same observations"""
    new = _plant(state, action)
    new[0] += np.float32(0.005 * b)
    return new.astype(np.float32)


# ------------------------------------------------------------------------------------------------ the filter alone
# family, uncertain parameters (P columns), Mp
FILTERS = [
    ("pendulum", ("length",), 1), ("pendulum", ("length", "mass"), 65), ("pendulum", ("g", "length", "mass"), 3), ("particle", ("mass",), 48),
    ("skid_steer", ("x_icr", "wheel_radius", "axial_distance"), 130), ("skid_steer", ("wheel_radius",), 3),
    ("cartpole", ("mass_pole", "length", "mass_cart", "f_mag"), 48), ("cartpole", ("length", "mass_pole"), 130),
]
CENTRE = dict(length=1.0, mass=1.0, g=9.8, x_icr=0.2, wheel_radius=0.0625, axial_distance=0.475, mass_pole=1.0, mass_cart=1.0, f_mag=1.0)
STATE0 = dict(pendulum=[3.0, 0.0], particle=[-3.0, -3.0, 0.0, 0.0], skid_steer=[0.1, -0.2, 0.6, 0.3, 0.1], cartpole=[0.0, 0.1, 0.3, -0.2])


def _filters(family, up, Mp, optimizer="SGD", log_space=False):
    """B lone filters with their own particles and first observation, and a batch started from the same"""
    from dust_amd import MpfContext
    from oracle import grid_4x4_map

    P = len(up)
    centre = np.array([2.0 if (family == "particle" and k == "mass") else CENTRE[k] for k in up], np.float32)
    kw = dict(model=family, uncertain_params=up, obs_std=0.2, lr=1e-3 if optimizer == "Adam" else 1e-6, init_bw=0.05, optimizer=optimizer,
              log_space=log_space)
    if family == "particle":
        kw.update(grid=grid_4x4_map(), mass=2.0)
    if family == "skid_steer":
        kw.update(dt=0.1)
    if family == "cartpole":
        kw.update(dt=0.05)
    lone, xs, obs = [], [], []
    for b in range(B):
        rng = np.random.default_rng(300 + 10 * Mp + b)
        x0 = (centre * (1.0 + 0.05 * rng.standard_normal((Mp, P)))).astype(np.float32)
        if log_space:
            x0 = np.log(x0)
        o0 = (np.array(STATE0[family], np.float32) + 0.01 * rng.standard_normal(len(STATE0[family]))).astype(np.float32)
        lone.append(MpfContext(x0, o0, **kw))
        xs.append(x0)
        obs.append(o0)
    batch = lone[0].batch(B)
    batch.set_particles(np.stack(xs))
    batch.set_obs(np.stack(obs))
    return lone, batch, np.stack(obs)


@pytest.mark.parametrize("bw", [None, 0.03], ids=["silverman", "fixed"])
@pytest.mark.parametrize("family,up,Mp", FILTERS, ids=["%s-P%d-Mp%d" % (f, len(u), m) for f, u, m in FILTERS])
def test_batched_filter_equals_lone_filters(family, up, Mp, bw):
    """dust_mpf_batch_optimize on B = 3 environments against B lone MpfContext.optimize calls over three consecutive updates (optimiser
    step count and prior bandwidths carry over): particles, bw_used, grad_norms and the prior bandwidths, bit for bit.  Mp = 1, 3, 48
    (Mpad 64, R 16), 65 (Mpad 128, R 8: padded lanes), 130 (Mpad 192, R 4: a block of 768)."""
    lone, batch, obs = _filters(family, up, Mp)
    da = lone[0].da
    rng = np.random.default_rng(Mp)
    for t in range(3):
        acts = (0.5 * rng.standard_normal((B, da))).astype(np.float32)
        obs = (obs + 0.02 * rng.standard_normal(obs.shape)).astype(np.float32)
        gn, bwu = batch.optimize(acts, obs, bw, MPF_STEPS)
        for b, m in enumerate(lone):
            bw_b = m.silverman() if bw is None else bw
            gn_b = m.optimize(acts[b], obs[b], bw_b, MPF_STEPS)
            assert bwu[b] == np.float32(bw_b), (t, b, bwu[b], bw_b)
            assert np.array_equal(gn[b], gn_b), (t, b)
        x = batch.get_particles()
        pb = batch.get_prior_bw()
        for b, m in enumerate(lone):
            assert np.array_equal(x[b], m.get_particles()), (t, b)
            assert np.array_equal(pb[b], m.get_prior_bw()), (t, b)
        assert np.isfinite(x).all() and np.isfinite(gn).all()
    assert batch.stats()["calls"] == 3
    for o in lone + [batch]:
        o.close()


@pytest.mark.parametrize("family,up,Mp", [FILTERS[1], FILTERS[6]], ids=["pendulum", "cartpole"])
def test_batched_filter_carries_adam_state(family, up, Mp):
    """Adam through set_optimizer: the three state slots [B][Mp][P] and the step count persist across updates, per environment; a clone
    taken after the first update continues as its source does"""
    lone, batch, obs = _filters(family, up, Mp, optimizer="Adam")
    rng = np.random.default_rng(5)
    twin = None
    for t in range(3):
        acts = (0.5 * rng.standard_normal((B, lone[0].da))).astype(np.float32)
        obs = (obs + 0.02 * rng.standard_normal(obs.shape)).astype(np.float32)
        gn, _ = batch.optimize(acts, obs, None, MPF_STEPS)
        if twin is not None:
            gn2, _ = twin.optimize(acts, obs, None, MPF_STEPS)
            assert np.array_equal(gn, gn2) and np.array_equal(batch.get_particles(), twin.get_particles())
        for b, m in enumerate(lone):
            assert np.array_equal(gn[b], m.optimize(acts[b], obs[b], m.silverman(), MPF_STEPS)), (t, b)
            assert np.array_equal(batch.get_particles()[b], m.get_particles()), (t, b)
        if t == 0:
            twin = copy.deepcopy(batch)
    for o in lone + [batch, twin]:
        o.close()


@pytest.mark.parametrize("family,up,Mp", [FILTERS[1], FILTERS[3], FILTERS[5], FILTERS[7]], ids=["pendulum", "particle", "skid_steer", "cartpole"])
def test_batched_log_space_filter_equals_lone_filters(family, up, Mp):
    """the log-space instances of the batched kernel (a filter on its own may carry log parameters; the dual tick refuses one)"""
    lone, batch, obs = _filters(family, up, Mp, log_space=True)
    rng = np.random.default_rng(3)
    for t in range(2):
        acts = (0.5 * rng.standard_normal((B, lone[0].da))).astype(np.float32)
        obs = (obs + 0.02 * rng.standard_normal(obs.shape)).astype(np.float32)
        gn, bwu = batch.optimize(acts, obs, None, MPF_STEPS)
        x = batch.get_particles()
        for b, m in enumerate(lone):
            bw_b = m.silverman()
            assert np.array_equal(gn[b], m.optimize(acts[b], obs[b], bw_b, MPF_STEPS)) and bwu[b] == np.float32(bw_b), (t, b)
            assert np.array_equal(x[b], m.get_particles()), (t, b)
        assert np.isfinite(x).all() and np.isfinite(gn).all()
    for o in lone + [batch]:
        o.close()


@pytest.mark.parametrize("optimizer", ["SGD", "Adam"])
def test_inactive_filters_keep_everything(optimizer):
    """(Adam: the resumed environment's update depends on its state slots and its step count, which must not have moved while it was off)"""
    lone, batch, obs = _filters("pendulum", ("length", "mass"), 48, optimizer=optimizer)
    rng = np.random.default_rng(9)
    acts = (0.5 * rng.standard_normal((B, 1))).astype(np.float32)
    x0, pb0 = batch.get_particles(), batch.get_prior_bw()
    gn, bwu = batch.optimize(acts, obs + 0.01, None, MPF_STEPS, active=(1, 0, 1))
    x, pb = batch.get_particles(), batch.get_prior_bw()
    assert np.array_equal(x[1], x0[1]) and np.array_equal(pb[1], pb0[1]) and np.isnan(gn[1]).all() and np.isnan(bwu[1])
    for b in (0, 2):
        assert np.array_equal(gn[b], lone[b].optimize(acts[b], obs[b] + 0.01, lone[b].silverman(), MPF_STEPS))
        assert np.array_equal(x[b], lone[b].get_particles())
    # the middle environment's first update comes later and starts from ITS observation, step count and bandwidths
    gn, _ = batch.optimize(acts, obs + 0.02, None, MPF_STEPS, active=(0, 1, 0))
    assert np.array_equal(gn[1], lone[1].optimize(acts[1], obs[1] + 0.02, lone[1].silverman(), MPF_STEPS))
    assert np.array_equal(batch.get_particles()[1], lone[1].get_particles()) and np.array_equal(batch.get_particles()[0], x[0])
    for o in lone + [batch]:
        o.close()


# ------------------------------------------------------------------------------------------------ whole periods
def _batch_pair(family, mode, S, H, Mp, optimizer="SGD"):
    """B lone (context, filter) pairs with seed = SEEDS[b], and the two batches started from the same sequences, particles, observations"""
    pairs = [_pair(family, mode, S, H, Mp, seed=s) for s in SEEDS]
    if optimizer == "Adam":  # (state slots and a step count that enters the step: the batch copies both from its prototype)
        from dust_amd import _lib as L

        for _, m, _, _ in pairs:
            L.check(L.load().dust_mpf_set_optimizer(m._h, L.OPT_ADAM, 0.9, 0.999, 1e-8))
    if family == "nav":  # (that family's scenario - map, goal - follows the seed: every environment takes environment 0's, under its own noise seed)
        import amppi_cases as cases
        import skid_nav_cases as nav
        from dust_amd import Context

        sc = nav._S("amppi", "dual", 4000 + SEEDS[0], S=S, H=H, mode=dict(extended="extended", single="single", sigma="ut")[mode], up=UPS["nav"])
        for b in range(1, B):
            c_old, m, _, scale = pairs[b]
            c_old.close()
            c = Context(grid=nav.make_map(sc), seed=SEEDS[b], **nav.context_kwargs(sc))
            if mode == "sigma":
                c.set_param_weights(np.asarray(cases.weights(len(UPS["nav"]))[0], np.float32))
                c.set_sigma_scale(scale)
            pairs[b] = (c, m, pairs[0][2], scale)
    c0, m0, state0, scale = pairs[0]
    da = c0.da
    rng = np.random.default_rng(S + H + Mp)
    a0 = (0.3 * rng.standard_normal((B, H, da))).astype(np.float32)
    for b, (c, _, _, _) in enumerate(pairs):
        c.set_a_seq(a0[b])
    batch = c0.amppi_batch(B, seeds=SEEDS)
    batch.set_a_seq(a0)
    if scale is not None:
        batch.ctx.set_sigma_scale(scale)
    mb = m0.batch(B)
    mb.set_particles(np.stack([m.get_particles() for _, m, _, _ in pairs]))
    states = np.stack([p[2] + np.float32(0.01 * b) for b, p in enumerate(pairs)]).astype(np.float32)
    mb.set_obs(states)
    for b, (_, m, _, _) in enumerate(pairs):  # (the lone filters' first observation: the state their first period sees)
        m.condition(None, states[b])
    return pairs, batch, mb, states, rng


PERIODS = PIECES[:15] + [("pendulum", "extended", True, 1, 12, 1, 0.05), ("nav", "extended", False, 1000, 7, 3, None),
                         ("cartpole", "extended", True, 1000, 8, 48, None), ("particle", "extended", False, 1, 10, 3, None)]


@pytest.mark.parametrize("family,mode,device_noise,S,H,Mp,bw", PERIODS, ids=["-".join(str(v) for v in p) for p in PERIODS])
def test_batched_periods_equal_lone_periods(family, mode, device_noise, S, H, Mp, bw):
    """dust_amppi_dual_batch_tick on B = 3 against three lone dust_amppi_dual_tick calls over four periods (the first without a filter
    update), each environment under its own noise seed, prior key, plant, sequence and particles: costs, omega, a_seq before and after
    the roll, params_out, the filters' particles and bw_used, bit for bit"""
    pairs, batch, mb, states, rng = _batch_pair(family, mode, S, H, Mp)
    da = batch.da
    prev = None
    for t in range(4):
        actions = None if device_noise else (batch.get_a_seq()[:, None] + 0.5 * rng.standard_normal((B, S, H, da))).astype(np.float32)
        keys = [100 + t + (b << 32) for b in range(B)]
        costs, omega, aseq, rows, bwu = batch.dual_tick(mb, states, prev, actions, shared_params=mode == "single", mpf_steps=MPF_STEPS, mpf_bw=bw,
                                                        seeds=keys, roll=1, want_params=True)
        x, aseq_rolled = mb.get_particles(), batch.get_a_seq()
        for b, (c, m, _, _) in enumerate(pairs):
            c1, o1, a1, r1, bw1 = c.amppi_dual_tick(m, states[b], None if prev is None else prev[b], None if actions is None else actions[b],
                                                    shared_params=mode == "single", mpf_steps=MPF_STEPS, mpf_bw=bw, seed=keys[b], roll=1, want_params=True)
            assert np.array_equal(rows[b], r1), (t, b)
            assert np.array_equal(costs[b], c1) and np.array_equal(omega[b], o1) and np.array_equal(aseq[b], a1), (t, b)
            assert bwu[b] == np.float32(bw1), (t, b, bwu[b], bw1)
            assert np.array_equal(x[b], m.get_particles()), (t, b)
            assert np.array_equal(aseq_rolled[b], c.get_a_seq()), (t, b)
        assert np.isfinite(costs).all() and np.isfinite(aseq).all() and np.isfinite(x).all(), t
        prev = aseq[:, 0].copy()
        states = np.stack([_env_plant(b, states[b], prev[b]) for b in range(B)])
    pb = mb.get_prior_bw()
    for b, (c, m, _, _) in enumerate(pairs):
        assert np.array_equal(pb[b], m.get_prior_bw()), b
        c.close()
        m.close()
    batch.close()
    mb.close()


@pytest.mark.parametrize("optimizer", ["SGD", "Adam"])
def test_active_mask_skips_an_environment_and_resumes_it(optimizer):
    """the middle environment off for two periods, then on again: while off its particles, prior bandwidths and sequence stay, and once on
    it matches a lone pair that skipped the same periods - noise stream, and under Adam the three state slots and the step count (its
    bias corrections are powers of it: a count advanced or a slot written while off would show); the other two are unaffected, bit for bit"""
    pairs, batch, mb, states, _ = _batch_pair("pendulum", "extended", 257, 12, 48, optimizer=optimizer)
    last = [None] * B  # every environment's last applied action
    for t in range(5):
        on = np.array([1, 0 if t in (1, 2) else 1, 1], np.uint8)
        prev = None if t == 0 else np.stack([np.zeros(batch.da, np.float32) if a is None else a for a in last])
        keys = [500 + t + (b << 32) for b in range(B)]
        x0, pb0, a0 = mb.get_particles(), mb.get_prior_bw(), batch.get_a_seq()
        costs, omega, aseq, _, bwu = batch.dual_tick(mb, states, prev, None, mpf_steps=MPF_STEPS, seeds=keys, roll=1, active=on)
        x, pb, a1 = mb.get_particles(), mb.get_prior_bw(), batch.get_a_seq()
        for b, (c, m, _, _) in enumerate(pairs):
            if not on[b]:
                assert np.array_equal(x[b], x0[b]) and np.array_equal(pb[b], pb0[b]) and np.array_equal(a1[b], a0[b]), t
                assert np.isnan(costs[b]).all() and np.isnan(omega[b]).all() and np.isnan(aseq[b]).all() and np.isnan(bwu[b]), t
                continue
            c1, o1, s1, _, bw1 = c.amppi_dual_tick(m, states[b], None if prev is None else prev[b], None, mpf_steps=MPF_STEPS, seed=keys[b], roll=1)
            assert np.array_equal(costs[b], c1) and np.array_equal(omega[b], o1) and np.array_equal(aseq[b], s1), (t, b)
            assert bwu[b] == np.float32(bw1) and np.array_equal(x[b], m.get_particles()) and np.array_equal(a1[b], c.get_a_seq()), (t, b)
            last[b] = aseq[b, 0].copy()
            states[b] = _env_plant(b, states[b], last[b])
    for c, m, _, _ in pairs:
        c.close()
        m.close()
    batch.close()
    mb.close()


def _counts(nb):
    """profile and stats counters added by one period with a filter update at nb environments, extended mode, Silverman bandwidths"""
    from dust_amd import Context, MpfContext

    c = Context(model="pendulum", N=1, S=257, M=1, H=12, temperature=100.0, alpha=0.01, sigma_a=2.0, uncertain_params=("length", "mass"), seed=3)
    rng = np.random.default_rng(1)
    m = MpfContext((1.0 + 0.05 * rng.standard_normal((48, 2))).astype(np.float32), np.array([3.0, 0.0], np.float32), model="pendulum",
                   uncertain_params=("length", "mass"), obs_std=0.2, lr=1e-6, init_bw=0.05)
    batch, mb = c.amppi_batch(nb), m.batch(nb)
    states = np.tile(np.array([3.0, 0.0], np.float32), (nb, 1))
    keys = [1 + (b << 32) for b in range(nb)]
    aseq = batch.dual_tick(mb, states, seeds=keys, roll=1)[2]
    batch.ctx.profile(True)
    s0 = mb.stats()
    out = batch.dual_tick(mb, states + 0.01, aseq[:, 0].copy(), seeds=[k + 1 for k in keys], mpf_steps=MPF_STEPS, roll=1, want_outputs=False)
    assert all(o is None for o in out)  # (nothing read back: the call returned without waiting for the device)
    prof, s1 = batch.ctx.profile_get(), mb.stats()
    batch.ctx.profile(False)
    assert np.isfinite(batch.get_a_seq()).all() and np.isfinite(mb.get_particles()).all()
    for o in (batch, mb, c, m):
        o.close()
    return {k: v[1] for k, v in prof.items()}, {k: s1[k] - s0[k] for k in s0}


def test_launch_count_does_not_depend_on_B():
    p1, s1 = _counts(1)
    p5, s5 = _counts(5)
    assert p1 == p5 and s1 == s5, (p1, p5, s1, s5)
    assert p1["amppi_kernel"] == 1 and sum(p1.values()) == 2, p1  # (the tick and the roll)
    assert s1 == dict(launches=2, calls=1), s1  # (Silverman's rule and the update)


# ------------------------------------------------------------------------------------------------ the class
def _example():
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples", "amppi_dual_batch_example.py")
    spec = importlib.util.spec_from_file_location("amppi_dual_batch_example", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_class_equals_lone_objects_and_deepcopy_continues():
    """BatchDualAMPPI against B DualAMPPI(fused=True) objects over six periods of the example's scenario (S = 256, 32 filter particles),
    bit for bit; a deep copy taken after three periods continues as its source does"""
    ex = _example()
    kw = dict(n_envs=B, samples=256, horizon=12, mpf_particles=32, seed=2)
    loop, plant, start, _ = ex.scenario(**kw)
    lones = [ex.lone(b, **kw) for b in range(B)]
    states, ls = start.clone(), [s.reshape(1, -1) for _, _, s in lones]
    twin = None
    for t in range(6):
        if t == 3:
            twin, tstates = copy.deepcopy(loop), states.clone()
            assert twin._mb is not loop._mb and twin.controller._batch is not loop.controller._batch
        actions, states, omega = loop.tick(states, plant)
        if twin is not None:
            ta, tstates, tw = twin.tick(tstates, plant)
            assert torch.equal(ta, actions) and torch.equal(tstates, states) and torch.equal(tw, omega), t
        for b, (lo, pl, _) in enumerate(lones):
            a, ls[b], w = lo.tick(ls[b], pl)
            assert torch.equal(a, actions[b]) and torch.equal(w, omega[b]) and torch.equal(ls[b].reshape(-1), states[b]), (t, b)
            assert torch.equal(lo.last_costs, loop.last_costs[b]), (t, b)
            if t > 0:
                assert float(loop.last_bw[b]) == np.float32(lo.last_bw), (t, b)
    x = loop.dyn_particles
    assert torch.equal(x, twin.dyn_particles) and torch.equal(loop.a_seq, twin.a_seq)
    for b, (lo, _, _) in enumerate(lones):
        assert torch.equal(x[b], lo.dyn_particles) and torch.equal(loop.a_seq[b], lo.a_seq), b


def test_a_refused_call_keeps_the_keys_and_the_noted_update():
    from dust_amd import _lib as L

    loop, plant, start, _ = _example().scenario(n_envs=2, samples=64, horizon=8, mpf_particles=16, seed=5)
    _, states, _ = loop.tick(start, plant)
    t, pend = loop._t, loop._pending
    loop.roll = -1  # (dust_amppi_dual_batch_tick refuses a negative roll)
    with pytest.raises(L.DustError):
        loop.forward(states)
    assert loop._t == t and loop._pending is pend and pend is not None
    loop.roll = 1
    a_seq, _ = loop.forward(states)
    assert torch.isfinite(a_seq).all() and loop._t == t + 1 and loop._pending is None


def test_the_example_runs(capsys):
    states = _example().main(["--envs", "3", "--ticks", "3", "--samples", "64", "--horizon", "8", "--mpf-particles", "16"])
    assert states.shape == (4, 3, 2) and torch.isfinite(states).all()
    assert "3 ticks of 3 pendulums" in capsys.readouterr().out


# ------------------------------------------------------------------------------------------------ refusals
def test_refusals_come_before_any_launch():
    from dust_amd import Context, MpfContext
    from dust_amd import _lib as L
    from oracle import grid_4x4_map

    c, m, state, _ = _pair("pendulum", "extended", 64, 8, 16, seed=1)
    batch, mb = c.amppi_batch(2), m.batch(2)
    batch.ctx.profile(True)
    states = np.tile(state, (2, 1))
    keys = [1, 2]

    def refused(status, *a, **kw):
        with pytest.raises(L.DustError) as e:
            batch.dual_tick(*a, **kw)
        assert e.value.status == status, (e.value.status, str(e.value))

    def untouched():
        assert batch.ctx.profile_get() == {} and mb.stats() == dict(launches=0, calls=0)

    refused(L.ERR_UNSUPPORTED, mb, states, seeds=keys, flags=L.STORE_STATES)
    refused(L.ERR_UNSUPPORTED, mb, states, seeds=keys, flags=L.STORE_F16)
    refused(L.ERR_UNSUPPORTED, mb, states, seeds=keys, flags=L.EPS_F16)
    refused(L.ERR_INVALID, mb, states, seeds=keys, roll=-1)
    refused(L.ERR_INVALID, mb, states, seeds=None)
    mb3 = m.batch(3)
    refused(L.ERR_INVALID, mb3, states, seeds=keys)  # n_env differs
    mb3.close()
    m1 = MpfContext(np.ones((16, 1), np.float32), state, model="pendulum", uncertain_params=("length",))
    mb1 = m1.batch(2)
    refused(L.ERR_INVALID, mb1, states, seeds=keys)  # parameter columns differ (dual_pair_check)
    mb1.close()
    ml = MpfContext(np.zeros((16, 2), np.float32), state, model="pendulum", uncertain_params=("length", "mass"), log_space=True)
    mbl = ml.batch(2)
    refused(L.ERR_UNSUPPORTED, mbl, states, seeds=keys)  # a log-space filter
    mbl.close()
    untouched()
    for n in (0, 65536):
        with pytest.raises(L.DustError) as e:
            m.batch(n)
        assert e.value.status == L.ERR_INVALID
    noisy = MpfContext(np.full((16, 1), 2.0, np.float32), np.zeros(4, np.float32), model="particle", uncertain_params=("mass",), grid=grid_4x4_map(),
                       deterministic=False, noise_std=(0.1, 0.1))
    with pytest.raises(L.DustError) as e:
        noisy.batch(2)
    assert e.value.status == L.ERR_UNSUPPORTED
    # sigma weights without a scale, then with n_params != 2 P + 1
    cs = Context(model="pendulum", N=1, S=64, M=5, H=8, temperature=100.0, alpha=0.01, sigma_a=2.0, uncertain_params=("length", "mass"))
    cs.set_param_weights(np.full(5, 0.2, np.float32))
    bs = cs.amppi_batch(2)
    with pytest.raises(L.DustError) as e:
        bs.dual_tick(mb, states, seeds=keys)
    assert e.value.status == L.ERR_UNSUPPORTED
    # ... and weights and a scale with n_params = 3 over the filters' P = 2 columns (2 P + 1 = 5)
    c3 = Context(model="pendulum", N=1, S=64, M=3, H=8, temperature=100.0, alpha=0.01, sigma_a=2.0, uncertain_params=("length", "mass"))
    c3.set_param_weights(np.full(3, 1.0 / 3.0, np.float32))
    c3.set_sigma_scale(3.0)
    b3 = c3.amppi_batch(2)
    b3.ctx.set_sigma_scale(3.0)
    b3.ctx.profile(True)
    with pytest.raises(L.DustError) as e:
        b3.dual_tick(mb, states, seeds=keys)
    assert e.value.status == L.ERR_INVALID and b3.ctx.profile_get() == {}
    untouched()
    # a filter with more particle columns than its model has parameters has no batched form
    for model, up, cols, kw in (("particle", ("mass",), 2, dict(grid=grid_4x4_map(), mass=2.0)), ("pendulum", ("length", "mass"), 4, {})):
        wide = MpfContext(np.ones((16, cols), np.float32), np.zeros(4 if model == "particle" else 2, np.float32), model=model, uncertain_params=up, **kw)
        with pytest.raises(L.DustError) as e:
            wide.batch(2)
        assert e.value.status == L.ERR_UNSUPPORTED, model
        wide.close()
    # a refused update keeps the filters: nothing ran
    x0 = mb.get_particles()
    with pytest.raises(L.DustError):
        mb.optimize(None, states, 0.05, 4)  # an observation without the action that led to it
    assert np.array_equal(mb.get_particles(), x0) and mb.stats() == dict(launches=0, calls=0)
    for o in (b3, c3, bs, cs, noisy, ml, m1, batch, mb, c, m):
        o.close()
