"""The dual loop over an AMPPI controller on the device: dust_amppi_dual_tick (Context.amppi_dual_tick) and
dust_amd.controllers.DualAMPPI.  The fused period against its pieces called one by one through the C ABI (bit for bit), the in-kernel
parameter draws against the host's exact integer Philox, the launch count, the class's loop, deep copies and the refusals."""
import copy
import importlib.util
import os

import numpy as np
import pytest
import torch

import amppi_cases as cases
import philox_ref as px
import skid_nav_cases as nav

pytestmark = pytest.mark.gpu

MPF_STEPS = 4
PERIODS = 4
UPS = dict(pendulum=("length", "mass"), particle=("mass",), skid=("x_icr", "wheel_radius", "axial_distance"), nav=("wheel_radius", "axial_distance"),
           cartpole=("mass_pole", "length", "mass_cart", "f_mag"))
# centres of the filters' particles.  MPF's Silverman bandwidth pools every column (mpf.py:68-73), so columns of one scale keep the drawn rows
# physical: the cart-pole's four sampled parameters all lie round 1 here (a sampled value replaces the model's default)
CENTRE = dict(length=1.0, mass=1.0, x_icr=0.2, wheel_radius=0.0625, axial_distance=0.475, mass_pole=1.0, mass_cart=1.0, f_mag=1.0)


def _pair(family, mode, S, H, Mp, seed, log_space=False, up=None, mpf_up=None):
    """(context, filter, state0, sigma scale or None) of one family: an AMPPI context in the given mode and a filter over the same columns"""
    from dust_amd import Context, MpfContext
    from oracle import grid_4x4_map

    up = UPS[family] if up is None else up
    mpf_up = up if mpf_up is None else mpf_up
    P = len(up)
    cmode = dict(extended="extended", single="single", sigma="ut")[mode]
    if family == "nav":
        s = nav._S("amppi", "dual", 4000 + seed, S=S, H=H, mode=cmode, up=up)
        c = Context(grid=nav.make_map(s), seed=seed, **nav.context_kwargs(s))
        state0 = np.array(s["state0"], np.float32)
    else:
        s = cases.A("dual", family, S, H, cmode, up, seed)
        c = Context(grid=grid_4x4_map() if family == "particle" else None, seed=seed, **cases.context_kwargs(s))
        state0 = np.array(cases.FAMILY[family]["state0"], np.float32)
    scale = None
    if mode == "sigma":
        w, scale = cases.weights(P)
        c.set_param_weights(np.asarray(w, np.float32))
        c.set_sigma_scale(scale)
    rng = np.random.default_rng(900 + seed)
    centre = np.array([2.0 if (family == "particle" and k == "mass") else CENTRE[k] for k in mpf_up], np.float32)
    x0 = (centre * (1.0 + 0.05 * rng.standard_normal((Mp, len(mpf_up))))).astype(np.float32)
    if log_space:
        x0 = np.log(x0)
    model = dict(pendulum="pendulum", particle="particle", skid="skid_steer", nav="skid_steer", cartpole="cartpole")[family]
    kw = dict(model=model, uncertain_params=mpf_up, log_space=log_space, obs_std=0.2, lr=1e-6, init_bw=0.05)
    if family == "particle":
        kw.update(grid=grid_4x4_map(), mass=2.0)
    if family in ("skid", "nav"):
        kw.update(dt=0.1)
    if family == "cartpole":
        kw.update(dt=0.05)
    m = MpfContext(x0, state0, **kw)
    return c, m, state0, scale


def _plant(state, action):
    """a small host plant: any deterministic map does - both sides see the same observations"""
    new = state.copy()
    new[: action.size] += np.float32(0.02) * np.tanh(action)
    new[-1] += np.float32(0.01)
    return new.astype(np.float32)


# family, mode, device noise, S, H, Mp, fixed bandwidth (None: Silverman's rule)
PIECES = [
    ("pendulum", "extended", False, 257, 12, 48, None), ("pendulum", "single", True, 257, 12, 3, 0.05), ("pendulum", "sigma", False, 257, 12, 1, 0.05),
    ("particle", "extended", True, 257, 10, 3, None), ("particle", "single", False, 257, 10, 48, None), ("particle", "sigma", True, 257, 10, 48, 0.05),
    ("skid", "extended", False, 257, 7, 3, 0.01), ("skid", "single", True, 257, 7, 48, None), ("skid", "sigma", False, 257, 7, 3, None),
    ("nav", "extended", True, 257, 7, 48, None), ("nav", "single", False, 257, 7, 1, 0.01), ("nav", "sigma", True, 257, 7, 48, None),
    ("cartpole", "extended", False, 257, 8, 48, None), ("cartpole", "single", True, 257, 8, 3, 0.01), ("cartpole", "sigma", False, 257, 8, 48, None),
    ("pendulum", "extended", True, 1, 12, 1, 0.05), ("skid", "extended", True, 64, 7, 48, None), ("nav", "extended", False, 1000, 7, 3, None),
    ("cartpole", "extended", True, 1000, 8, 1, 0.02), ("particle", "extended", False, 64, 10, 48, None),
]


@pytest.mark.parametrize("family,mode,device_noise,S,H,Mp,bw", PIECES, ids=["-".join(str(v) for v in p) for p in PIECES])
def test_fused_period_equals_its_pieces(family, mode, device_noise, S, H, Mp, bw):
    """dust_amppi_dual_tick against silverman, mpf.optimize, prior_sample / sigma_points, amppi_update(params=...), amppi_roll called one by
    one with the same Philox key: bit-identical costs, weights, sequences, filter particles and bandwidths over four periods, and
    params_out equal to the rows dust_mpf_prior_sample gives (the rows the in-kernel draws used)"""
    ca, ma, state, scale = _pair(family, mode, S, H, Mp, seed=7)
    cb, mb, _, _ = _pair(family, mode, S, H, Mp, seed=7)
    da = ca.da
    rng = np.random.default_rng(S + H + Mp)
    a0 = (0.3 * rng.standard_normal((H, da))).astype(np.float32)
    ca.set_a_seq(a0)
    cb.set_a_seq(a0)
    prev = None
    for t in range(PERIODS):
        actions = None if device_noise else (cb.get_a_seq()[None] + 0.5 * rng.standard_normal((S, H, da))).astype(np.float32)
        seed = 100 + t
        costs1, omega1, aseq1, rows1, bw1 = ca.amppi_dual_tick(ma, state, prev, actions, shared_params=mode == "single", mpf_steps=MPF_STEPS, mpf_bw=bw,
                                                              seed=seed, roll=1, want_params=True)
        if prev is not None:
            bw2 = mb.silverman() if bw is None else bw
            mb.optimize(prev, state, bw2, MPF_STEPS)
            assert bw1 == np.float32(bw2), (t, bw1, bw2)
        else:
            assert bw1 == 0.0
        rows2 = mb.sigma_points(scale) if mode == "sigma" else mb.prior_sample(1 if mode == "single" else S, seed)
        costs2, omega2, aseq2, _, _ = cb.amppi_update(state, actions, rows2, shared_params=mode == "single")
        cb.amppi_roll(1)
        assert np.array_equal(rows1, rows2), t
        assert np.array_equal(costs1, costs2) and np.array_equal(omega1, omega2) and np.array_equal(aseq1, aseq2), t
        assert np.isfinite(costs1).all() and np.isfinite(aseq1).all(), t
        assert np.array_equal(ma.get_particles(), mb.get_particles()), t
        assert np.array_equal(ca.get_a_seq(), cb.get_a_seq()), t  # (after the roll)
        prev = aseq1[0].copy()
        state = _plant(state, prev)
    assert np.array_equal(ma.get_prior_bw(), mb.get_prior_bw())
    for o in (ca, cb, ma, mb):
        o.close()


def test_component_index_is_the_hosts():
    """S = 257, Mp = 3, P = 2, component means 100 bw apart: the component of row s is (philox4x32_10(s, 0x6d7066, 0, 0; seed)[0] Mp) >> 32
    in exact integer arithmetic (tests/philox_ref.py), and |z| < 6 for every draw of this seed (checked on the host replica of
    philox_normal4 below: with 24-bit uniforms sqrt(-2 ln 2^-25) = 5.89 bounds it for any seed), so every row lies within 6 bw of ITS mean"""
    from dust_amd import Context, MpfContext

    S, Mp, P, bw, seed = 257, 3, 2, 0.01, 20260
    s = cases.A("dual_k", "pendulum", S, 8, "extended", ("length", "mass"), 1)
    c = Context(**cases.context_kwargs(s))
    means = (1.0 + 100.0 * bw * np.arange(Mp)[:, None] * np.ones((1, P))).astype(np.float32)
    m = MpfContext(means, np.array([3.0, 0.0], np.float32), model="pendulum", uncertain_params=("length", "mass"), init_bw=bw)
    ctr = np.zeros((S, 4), np.uint64)
    ctr[:, 0], ctr[:, 1] = np.arange(S), 0x6D7066
    k = ((px.philox4x32_10(ctr, seed)[:, 0].astype(np.uint64) * np.uint64(Mp)) >> np.uint64(32)).astype(np.int64)
    assert set(k.tolist()) == {0, 1, 2}
    ctr[:, 1], ctr[:, 2] = 0x6D7067, 1
    z = px.normal4(ctr, seed)[:, :P]
    assert np.abs(z).max() < 6.0
    rows = c.amppi_dual_tick(m, np.array([3.0, 0.0], np.float32), seed=seed, want_params=True)[3]
    assert rows.shape == (S, P)
    assert (np.abs(rows - means[k]) <= 6.0 * bw).all()
    # (and the draw itself against the host's float64 Box-Muller: half an ulp of 3 is 1.2e-7, the device's fp32 log / sin / cos add < 1e-7)
    assert np.abs(rows - (means[k] + bw * z)).max() < 1e-6
    assert np.array_equal(rows, m.prior_sample(S, seed))
    c.close()
    m.close()


def test_one_period_is_one_launch():
    """extended mode: the period adds exactly one kernel to the controller's profile (the draws are inside it), no parameter rows come
    back unless asked for"""
    c, m, state, _ = _pair("nav", "extended", 257, 7, 48, seed=3)
    c.profile(True)
    out = c.amppi_dual_tick(m, state, seed=5, roll=1)
    prof = c.profile_get()
    assert list(prof) == ["amppi_kernel"] and prof["amppi_kernel"][1] == 1, prof
    assert out[3] is None
    a0 = out[2][0].copy()
    c.amppi_dual_tick(m, _plant(state, a0), a0, seed=6, roll=1, mpf_steps=MPF_STEPS, want_outputs=False)  # (nothing read back: stays asynchronous)
    prof = c.profile_get()
    assert list(prof) == ["amppi_kernel"] and prof["amppi_kernel"][1] == 2, prof
    assert np.isfinite(c.get_a_seq()).all() and np.isfinite(m.get_particles()).all()
    c.close()
    m.close()


# ------------------------------------------------------------------------------------------------ the class
def _example():
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples", "amppi_dual_example.py")
    spec = importlib.util.spec_from_file_location("amppi_dual_example", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _host_plant(plant):
    return lambda x, u: plant.step(x.reshape(1, -1), u.reshape(1, -1))


def test_dual_amppi_fused_runs_the_examples_loop():
    """DualAMPPI(fused=True), own draws, 6 periods of examples/amppi_dual_example.py at S = 256: finite outputs, normalised weights,
    Silverman bandwidths of the particles each update started from, and reading dyn_particles between step() and forward() carries
    the noted update out first"""
    from dust_amd.inference.mpf import silvermans_rule

    loop, plant, start, _, _ = _example().scenario(samples=256, horizon=12, mpf_particles=32, seed=1, mpf_bw=None)
    state = start.reshape(1, -1)
    step = _host_plant(plant)
    for t in range(6):
        x_before = loop.mpf.x.clone()  # (the filter itself: the property would flush)
        pending = loop._pending is not None
        assert pending == (t > 0)
        a_seq, omega = loop.forward(state)
        assert a_seq.shape == (12, 2) and omega.shape == (256,)
        assert torch.isfinite(a_seq).all() and torch.isfinite(omega).all() and torch.isfinite(loop.last_costs).all()
        assert abs(float(torch.logsumexp(omega.double(), 0))) < 1e-5
        if pending:
            want = silvermans_rule(x_before.view(-1, 1).numpy()) * loop.mpf.bw_scale
            assert abs(loop.last_bw - want) <= 1e-6 * want, (t, loop.last_bw, want)  # (float64 on the device, rounded once to fp32: 6e-8)
            assert not torch.equal(loop.mpf.x, x_before), "the filter update ran inside forward()"
        state = step(state, a_seq[0])
        loop.step(a_seq[0], state)
    assert loop._pending is not None
    x_before = loop.mpf.x.clone()
    x_now = loop.dyn_particles
    assert loop._pending is None and not torch.equal(x_now, x_before) and torch.isfinite(x_now).all()


@pytest.mark.parametrize("fused", [True, False])
def test_deepcopy_mid_loop_continues_bit_identically(fused):
    loop, plant, start, _, _ = _example().scenario(samples=256, horizon=12, mpf_particles=32, seed=2, fused=fused)
    state = start.reshape(1, -1)
    step = _host_plant(plant)
    for _ in range(2):
        _, state, _ = loop.tick(state, step)
    twin = copy.deepcopy(loop)
    assert twin.controller._ctx is not loop.controller._ctx and twin.mpf._dev is not loop.mpf._dev
    assert twin.mpf.prior._seed == loop.mpf.prior._seed  # (the unfused draws are keyed by the prior's own counter: the copy carries it)
    sa = sb = state
    for _ in range(3):
        aa, sa, wa = loop.tick(sa, step)
        ab, sb, wb = twin.tick(sb, step)
        assert torch.equal(aa, ab) and torch.equal(sa, sb) and torch.equal(wa, wb)
    assert torch.equal(loop.dyn_particles, twin.dyn_particles) and torch.equal(loop.a_seq, twin.a_seq)


def test_fused_sigma_and_single_modes_run_through_the_class():
    """the staged modes through DualAMPPI(fused=True): a MerweScaledUTF controller (the prior's sigma points, computed on the device) and
    "single" (one staged row); their bits are pinned by test_fused_period_equals_its_pieces, here the class reaches them"""
    from dust_amd.utils.utf import MerweScaledUTF

    ex = _example()
    for sampling in (MerweScaledUTF(n=1, alpha=1.0), "single"):
        loop, plant, start, _, _ = ex.scenario(samples=64, horizon=8, mpf_particles=16, seed=4, sampling=sampling)
        state, step = start.reshape(1, -1), _host_plant(plant)
        x0 = loop.mpf.x.clone()
        for _ in range(3):
            a, state, w = loop.tick(state, step)
            assert torch.isfinite(a).all() and abs(float(torch.logsumexp(w.double(), 0))) < 1e-5
        assert loop.last_bw is not None and not torch.equal(loop.dyn_particles, x0)


def test_fused_and_unfused_class_agree_at_seed_0():
    """at seed = 0 both forms key their draws 1, 2, ...; with a fixed filter bandwidth (the host's and the device's Silverman rule may differ
    in the last bit) the one-call period and the hand composition give the same bits - period order, roll placement, which prior the rows
    come from"""
    ex = _example()
    recs = []
    for fused in (True, False):
        loop, plant, start, _, _ = ex.scenario(samples=256, horizon=12, mpf_particles=32, seed=0, fused=fused)
        loop.mpf_bw = 0.004
        state, step, rec = start.reshape(1, -1), _host_plant(plant), []
        for _ in range(4):
            a_seq, omega = loop.forward(state)
            state = step(state, a_seq[0])
            loop.step(a_seq[0], state)
            rec.append((a_seq, omega, loop.last_costs))
        rec.append((loop.dyn_particles, loop.a_seq))
        recs.append(rec)
    for t, (x, y) in enumerate(zip(*recs)):
        for u, v in zip(x, y):
            assert torch.equal(u, v), t


def test_a_refused_fused_call_keeps_the_key_and_the_noted_update():
    from dust_amd import _lib as L

    loop, plant, start, _, _ = _example().scenario(samples=64, horizon=8, mpf_particles=16, seed=5)
    state = start.reshape(1, -1)
    _, state, _ = loop.tick(state, _host_plant(plant))
    seed, pend, roll = loop._seed, loop._pending, loop.roll
    loop.roll = -1  # (dust_amppi_dual_tick refuses a negative roll)
    with pytest.raises(L.DustError):
        loop.forward(state)
    assert loop._seed == seed and loop._pending is pend and pend is not None
    loop.roll = roll
    a_seq, _ = loop.forward(state)
    assert torch.isfinite(a_seq).all() and loop._seed == seed + 1 and loop._pending is None


def test_the_example_runs(capsys):
    states = _example().main(["--ticks", "3", "--samples", "64", "--horizon", "8", "--mpf-particles", "16"])
    assert states.shape == (4, 5) and torch.isfinite(states).all()
    out = capsys.readouterr().out
    assert "3 ticks: distance to the goal" in out and "wheel_radius estimate" in out


# ------------------------------------------------------------------------------------------------ the reference's composed loop
def _fixture_loop(s, g, fused=False):
    """DualAMPPI over the repo's mirror classes of scenario s, its filter started from the fixture's particles"""
    import amppi_dual_cases as dc
    import test_gpu_amppi as ta
    from dust_amd.controllers import DualAMPPI
    from dust_amd.inference import MPF, GaussianLikelihood

    flt = dc.FILTER[s["family"]]
    model, inst, term = ta._mirror(s, g)
    ctrl = ta._controller(s, g, model, inst, term)
    fmodel = ta._mirror(s, g)[0]
    mpf = MPF(init_particles=torch.tensor(g["x0"]), likelihood=GaussianLikelihood(initial_obs=torch.tensor(g["state"]), obs_std=flt["obs_std"], model=fmodel,
                                                                                log_space=False),
              optimizer_class=torch.optim.SGD, lr=flt["lr"], bw=s["bw"] if s["bw"] else 0.1, bw_scale=1.0)
    return DualAMPPI(ctrl, model, mpf, mpf_bw=s["bw"], mpf_steps=s["mpf_steps"], fused=fused, roll=1), model


def _near(got, g, q, k):
    from helpers import elemerr

    return min(elemerr(got, g[q][k]), elemerr(got, g[q + "_f64"][k]))


def _run_fixture(name, golden, fused):
    """four periods of fixture `name` through DualAMPPI from the recorded actions (and rows, where the mode draws any) and the plant's
    recorded states -> per period dict(costs, omega, a_seq1, x, bw).  The fused class carries period k's filter update out inside the
    forward() of period k + 1: its particles and bandwidth are read there (the last one through dyn_particles)"""
    import amppi_dual_cases as dc
    import test_gpu_amppi as ta

    s, g = dc.BY_TAG[name], golden("amppi_dual_" + name)
    loop, model = _fixture_loop(s, g, fused=fused)
    state, T, got = torch.tensor(g["state"]), int(g["T"]), []
    for k in range(T):
        if "params" in g:
            ta._feed(model, g["params"][k])
        a_seq, omega = loop.forward(state, torch.tensor(g["actions"][k]))
        if fused and k > 0:
            assert loop._pending is None
            got[k - 1].update(x=loop.mpf.x.numpy(), bw=np.array([loop.last_bw]))
        got.append(dict(costs=loop.last_costs.numpy(), omega=omega.numpy(), a_seq1=a_seq.numpy()))
        state = torch.tensor(g["plant"][k])
        _, bw = loop.step(a_seq[0], state)
        if not fused:
            got[k].update(x=loop.dyn_particles.numpy(), bw=np.array([bw]))
        else:
            assert loop._pending is not None
    if fused:
        got[T - 1].update(x=loop.dyn_particles.numpy(), bw=np.array([loop.last_bw]))
    return s, g, got


def _check_fixture(name, s, g, got):
    import amppi_dual_cases as dc
    from helpers import elemerr

    for k, gk in enumerate(got):
        errs = {q: _near(v, g, q, k) for q, v in gk.items()}
        print(name, k, "  ".join("%s %.1e/%.1e" % (q, e, float(g["tol_" + q][k])) for q, e in errs.items()))
        for q, e in errs.items():
            assert e <= float(g["tol_" + q][k]), (k, q, e)
        for v in dc.variants_of(s):
            if v == "stale" and k == 0:
                continue
            assert elemerr(gk["costs"], g["costs_" + v][k]) >= 9 * float(g["tol_costs"][k]), (k, v)  # (10 tol from the truth, the truth within 1)


@pytest.mark.parametrize("name", ["pend_ext", "part_ext", "cart_single", "skid_ut"])
def test_fixture_through_the_unfused_class(golden, name):
    """the reference's own MPF.optimize and AMPPI.update_actions composed over four periods (tests/golden/amppi_dual_<tag>.npz) against
    DualAMPPI(fused=False) from the recorded actions, with model.sample_params handing out the recorded rows and the plant's recorded
    states: per period costs, weights, the sequence, the filter's particles and the bandwidth within the stored tolerances - and the
    costs >= 10 tolerances away from every power variant (a wrong period order, roll placement or stale rows would land there)"""
    _check_fixture(name, *_run_fixture(name, golden, fused=False))


def test_sigma_point_fixture_through_the_fused_call(golden):
    """the sigma-point fixture through DualAMPPI(fused=True) with the recorded actions: that mode draws nothing, so dust_amppi_dual_tick
    itself - the filter update, the sigma points of the refreshed prior computed on the device, the update, the roll - is held to the
    reference's numbers, and away from its power variants (costs_stale: the points of the prior before the period's filter update)"""
    s, g, got = _run_fixture("skid_ut", golden, fused=True)
    _check_fixture("skid_ut fused", s, g, got)
    # and the staged points themselves, through the C ABI on a filter holding the reference's particles of each period
    from dust_amd import Context, MpfContext

    c = Context(**cases.context_kwargs(dict(s, mode="ut")))
    c.set_param_weights(g["loc_weights"])
    c.set_sigma_scale(float(g["sigma_scale"]))
    for k in range(int(g["T"])):
        x = g["x0"] if k == 0 else g["x"][k - 1]
        m = MpfContext(x, g["state"], model="skid_steer", uncertain_params=s["up"], init_bw=float(s["bw"]), dt=0.1)
        rows = c.amppi_dual_tick(m, g["state"], actions=g["actions"][k], want_params=True)[3]
        assert _near(rows, g, "sigma_points", k) <= float(g["tol_sigma_points"][k]), k
        m.close()
    c.close()


# ------------------------------------------------------------------------------------------------ refusals
def test_refusals():
    from dust_amd import Context, MpfContext, _lib as L

    def status(fn):
        with pytest.raises(L.DustError) as e:
            fn()
        assert str(e.value)
        return e.value.status

    def tick(c, m, state, **kw):
        try:
            return status(lambda: c.amppi_dual_tick(m, state, seed=1, **kw))
        finally:
            c.close()
            m.close()

    # a context that is not an AMPPI one
    s = cases.A("r", "pendulum", 64, 8, "extended", ("length", "mass"), 1)
    c, m, st, _ = _pair("pendulum", "extended", 64, 8, 8, 1)
    c.close()
    assert tick(Context(**cases.context_kwargs(s, N=2)), m, st) == L.ERR_INVALID
    # dim_p != P, and "none"
    c, m, st, _ = _pair("pendulum", "extended", 64, 8, 8, 1, up=("length",), mpf_up=("length", "mass"))
    assert tick(c, m, st) == L.ERR_INVALID
    c, m, st, _ = _pair("pendulum", "extended", 64, 8, 8, 1)
    c.close()
    assert tick(Context(**cases.context_kwargs(cases.A("r", "pendulum", 64, 8, "none", (), 1))), m, st) == L.ERR_INVALID
    # other devices: only where a second one exists
    if torch.cuda.device_count() > 1:
        c, m, st, _ = _pair("pendulum", "extended", 64, 8, 8, 1)
        c.close()
        assert tick(Context(**cases.context_kwargs(s, device=1)), m, st) == L.ERR_INVALID
    # different parameters / column orders
    c, m, st, _ = _pair("skid", "extended", 64, 7, 8, 1, up=("x_icr", "wheel_radius"), mpf_up=("wheel_radius", "x_icr"))
    assert tick(c, m, st) == L.ERR_INVALID
    c, m, st, _ = _pair("nav", "extended", 64, 7, 8, 1, up=("x_icr", "wheel_radius"), mpf_up=("x_icr", "axial_distance"))
    assert tick(c, m, st) == L.ERR_INVALID
    c, m, st, _ = _pair("cartpole", "extended", 64, 8, 8, 1, up=("mass_pole", "length"), mpf_up=("length", "mass_pole"))
    assert tick(c, m, st) == L.ERR_INVALID
    c, m, st, _ = _pair("cartpole", "extended", 64, 8, 8, 1, up=("mass_pole", "length"))
    m.close()
    m = MpfContext(np.ones((8, 2), np.float32), np.array([3.0, 0.0], np.float32), model="pendulum", uncertain_params=("length", "mass"))
    assert tick(c, m, st) == L.ERR_INVALID  # a cart-pole controller takes a cart-pole filter
    # a log-space filter; a log-space controller
    c, m, st, _ = _pair("pendulum", "extended", 64, 8, 8, 1, log_space=True)
    assert tick(c, m, st) == L.ERR_UNSUPPORTED
    c, m, st, _ = _pair("pendulum", "extended", 64, 8, 8, 1)
    c.close()
    assert tick(Context(**cases.context_kwargs(s, params_log_space=True)), m, st) == L.ERR_UNSUPPORTED
    # sigma weights without a scale, or with M != 2P + 1
    c, m, st, _ = _pair("pendulum", "sigma", 64, 8, 8, 1)
    c.set_sigma_scale(0.0)
    assert tick(c, m, st) == L.ERR_UNSUPPORTED
    c, m, st, _ = _pair("pendulum", "extended", 64, 8, 8, 1)
    c.close()
    c = Context(**cases.context_kwargs(s, M=3))
    c.set_param_weights(np.array([0.0, 0.5, 0.5], np.float32))
    c.set_sigma_scale(2.0)
    assert tick(c, m, st) == L.ERR_INVALID
    c, m, st, _ = _pair("pendulum", "extended", 64, 8, 8, 1)
    c.close()
    assert tick(Context(**cases.context_kwargs(s, M=3)), m, st) == L.ERR_INVALID  # n_params > 1 without weights
    # what dust_amppi_update refuses: Particle with velocity control
    c, m, st, _ = _pair("particle", "extended", 64, 10, 8, 1)
    c.close()
    ps = cases.A("r", "particle", 64, 10, "extended", ("mass",), 1)
    from oracle import grid_4x4_map

    cv = Context(grid=grid_4x4_map(), **cases.context_kwargs(ps, control_type="velocity", target=(4.0, 4.5), w_state=(0.5, 0.5), w_term=(1.0, 1.0)))
    assert tick(cv, m, np.zeros(2, np.float32)) == L.ERR_UNSUPPORTED
    # bad step counts
    c, m, st, _ = _pair("pendulum", "extended", 64, 8, 8, 1)
    assert tick(c, m, st, roll=-1) == L.ERR_INVALID
    # (dust_amppi_dual_tick also refuses a filter of more than 1024 particles or over more than 4 parameters: dust_mpf_create makes no such
    # filter - "MPF supports 1..1024 particles" -, so that arm cannot be reached from here)


def test_a_sharded_context_is_refused(monkeypatch):
    """a context with a communicator forced through the sharded path (the way of test_c_side_rccl_tick_world1): through the C ABI and
    through the class"""
    from dust_amd import Context, _lib as L

    monkeypatch.setenv("DUST_COMM_FORCE", "1")
    s = cases.A("r", "pendulum", 64, 8, "extended", ("length", "mass"), 1)
    c, m, st, _ = _pair("pendulum", "extended", 64, 8, 8, 1)
    c.close()
    c = Context(shard_offset=0, shard_size=1, **cases.context_kwargs(s))
    c.comm_init(Context.comm_unique_id(), 0, 1)
    with pytest.raises(L.DustError) as e:
        c.amppi_dual_tick(m, st, seed=1)
    assert e.value.status == L.ERR_UNSUPPORTED and "sharded" in str(e.value)
    # the class: its context, made sharded the same way
    loop, plant, start, _, _ = _example().scenario(samples=64, horizon=8, mpf_particles=16, seed=6)
    ctx = loop.controller._ensure_ctx(loop.model)
    ctx.comm_init(Context.comm_unique_id(), 0, 1)
    with pytest.raises(L.DustError) as e:
        loop.forward(start)
    assert e.value.status == L.ERR_UNSUPPORTED
    c.close()
    m.close()


def test_class_refusals_on_the_device():
    """the constructor refuses a log-space filter and params_sampling="none" (tests/test_amppi_dual_cpu.py has them without a device: here
    with a real filter)"""
    from dust_amd.controllers import AMPPI, DualAMPPI
    from dust_amd.costs import PendulumQuadCos
    from dust_amd.inference import MPF, GaussianLikelihood
    from dust_amd.models import PendulumModel

    model, pc = PendulumModel(uncertain_params=("length",)), PendulumQuadCos()
    mk = lambda sampling: AMPPI(model.observation_space, model.action_space, 8, 64, inst_cost_fn=pc.inst_cost, term_cost_fn=pc.term_cost,
                                params_sampling=sampling)
    x0 = torch.ones(8, 1) + 0.1 * torch.arange(8.0).reshape(-1, 1)
    mpf = lambda log: MPF(init_particles=x0.log() if log else x0, likelihood=GaussianLikelihood(initial_obs=torch.tensor([3.0, 0.0]), obs_std=0.1, model=model,
                                                                                              log_space=log), optimizer_class=torch.optim.SGD, lr=1e-3, bw=0.1)
    with pytest.raises(NotImplementedError, match="log-space"):
        DualAMPPI(mk("extended"), model, mpf(True))
    with pytest.raises(ValueError, match="none"):
        DualAMPPI(mk("none"), model, mpf(False))
    loop = DualAMPPI(mk("extended"), model, mpf(False), mpf_bw=0.1, mpf_steps=2, fused=True)
    a_seq, omega = loop.forward(torch.tensor([3.0, 0.0]))
    assert a_seq.shape == (8, 1) and omega.shape == (64,)
    # controller and filter naming different columns: the fused call refuses (as dust_dual_tick does), through the class
    from dust_amd import _lib as L
    from dust_amd.costs import QuadraticCost
    from dust_amd.models import SkidSteerRobot

    cm = SkidSteerRobot(0.1, uncertain_params=("x_icr", "wheel_radius"))
    fm = SkidSteerRobot(0.1, uncertain_params=("wheel_radius", "x_icr"))
    qc = QuadraticCost((1.0, 0.5, 0.0, 0.0, 0.0), (1.0, 1.0, 0.1, 0.0, 0.0))
    ctrl = AMPPI(cm.observation_space, cm.action_space, 8, 64, inst_cost_fn=qc.inst_cost, term_cost_fn=qc.term_cost, params_sampling="extended")
    x2 = torch.tensor([0.0625, 0.2]) * (1.0 + 0.05 * torch.arange(8.0).reshape(-1, 1))
    flt = MPF(init_particles=x2, likelihood=GaussianLikelihood(initial_obs=torch.zeros(5), obs_std=0.1, model=fm, log_space=False),
              optimizer_class=torch.optim.SGD, lr=1e-6, bw=0.01)
    with pytest.raises(L.DustError) as e:
        DualAMPPI(ctrl, cm, flt, mpf_bw=0.01, fused=True).forward(torch.zeros(5))
    assert e.value.status == L.ERR_INVALID and "column order" in str(e.value)
