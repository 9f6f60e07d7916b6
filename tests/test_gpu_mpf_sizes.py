"""The dynamics filter (dust_amd/csrc/mpf.hpp) beyond 12 particles, against something independent of it.

Three forms of the optimisation kernel are compared everywhere they are eligible:
  single   mpf_optimize_kernel, one workgroup (DUST_MPF_GRID=0)
  poll     mpf_optimize_poll_kernel<P, KC>, the data-polled grid (the default from 96 particles; KC = 4 / 8 / 16 by particle count)
  counter  mpf_optimize_grid_kernel, the counter grid (DUST_MPF_POLL=0)
(DUST_MPF_GRID=1 sends 8 ... 95 particles through the grid forms as well.)  The switches are read once, in dust_mpf_create, so they are set
before the context is made; every test asserts stats(), so which kernel produced the compared numbers is on record.

  * test_fixture_*: the reference's own filter (tests/golden/mpf_sz_*.npz, made by tests/golden/make_golden_mpf_sizes.py) - the Jacobian
    branches only autograd can vouch for, at 70 ... 1 024 particles.  Tolerances are the fixture's, measured from the reference alone.
  * test_size_sweep_vs_oracle: every edge of the launch geometry, against the CPU oracle, at TOL.
  * test_grid_optimisers_follow_torch: momentum SGD, RMSprop, Adagrad and AdamW inside both grid forms against torch.optim on the host.
  * test_prior_log_prob_vs_float64: the prior's density against a float64 log-sum-exp.

Two-step calls are compared by DISPLACEMENT x_2 - x0, not position: a step moves a particle of order 1 by 1e-3 ... 1e-2, so a position
compared at 1e-5 would hide a 0.1 % fault of phi.  The displacement's tolerance is the position's times rms(x_2) / rms(x_2 - x0).
"""
import functools

import numpy as np
import pytest
import torch

from helpers import MPF_SIZE_CASES, elemerr, mpf_size_disp_err, mpf_size_err

pytestmark = pytest.mark.gpu

TOL = 1e-5
# Ceiling of a displacement tolerance TOL * rms(x) / rms(displacement): the steps must move the particles by at least 0.5 % of their rms,
# or the scaled bound says nothing about phi (a case that barely moves would pass vacuously).  Step sizes below are chosen so it holds.
DISP_TOL_MAX = 2e-3
FORMS = ("single", "poll", "counter")


def _set_form(monkeypatch, form, Mp):
    """the development switches that select `form` for a context of Mp particles (to be created next)"""
    monkeypatch.delenv("DUST_MPF_GRID_TEST", raising=False)
    monkeypatch.delenv("DUST_MPF_GRID", raising=False)
    monkeypatch.delenv("DUST_MPF_POLL", raising=False)
    if form == "single":
        monkeypatch.setenv("DUST_MPF_GRID", "0")
        return
    assert Mp >= 8, "the grid forms start at 8 particles"
    if Mp < 96:  # (below the default threshold: the grid form on request)
        monkeypatch.setenv("DUST_MPF_GRID", "1")
    if form == "counter":
        monkeypatch.setenv("DUST_MPF_POLL", "0")


def _served(m, form, calls):
    """which kernel served the optimize() calls so far"""
    want = {"grid": 0 if form == "single" else calls, "fallback": 0}
    assert m.stats() == want, (form, m.stats(), want)


def _rms(a):
    return float(np.sqrt(np.mean(np.asarray(a, np.float64) ** 2)))


# ------------------------------------------------------------------------------------------------ fixtures x forms
def _fixture_ctx(g, **kw):
    from dust_amd import MpfContext
    from oracle import grid_4x4_map

    kind = str(g["model_kind"])
    return MpfContext(g["x0"], g["obs0"], model=kind, uncertain_params=tuple(str(g["uncertain"]).split(",")), log_space=bool(int(g["log_space"])),
                      obs_std=float(g["obs_std"]), lr=float(g["lr"]), init_bw=float(g["bw"]), grid=grid_4x4_map() if kind == "particle" else None,
                      mass=2.0 if kind == "particle" else 1.0, optimizer=str(g["optimizer"]), **kw)


@pytest.mark.parametrize("name", MPF_SIZE_CASES)
def test_fixture_phi_vs_reference(golden, name):
    """dust_mpf_phi (the one-workgroup kernel with lr = 0: all it runs) against the reference's MPF.phi."""
    g = golden("mpf_sz_" + name)
    m = _fixture_ctx(g)
    m.condition(g["action"], g["obs1"])
    phi = m.phi(float(g["bw"]))
    e = mpf_size_err(phi, g, "phi0")
    print("%s phi0: err %.2e tol %.2e" % (name, e, float(g["tol_phi0"])))
    assert e < float(g["tol_phi0"])
    off = g["phi0_off"]  # the fixture has power: with its branch ignored the reference itself is >= 10 tolerances away
    assert elemerr(off, g["phi0"][:off.shape[0]]) >= 10 * float(g["tol_phi0"])
    assert np.array_equal(m.get_particles(), g["x0"])
    m.close()


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("name", MPF_SIZE_CASES)
def test_fixture_optimize_vs_reference(golden, name, form, monkeypatch):
    """A two-step optimize() (the shortest call the grid forms take; grad_norms[0] is the only direct view of a grid kernel's first phi)
    and two full calls, in every form, against the reference's MPF.optimize."""
    g = golden("mpf_sz_" + name)
    Mp, bw, n = int(g["Mp"]), float(g["bw"]), int(g["n_steps"])
    _set_form(monkeypatch, form, Mp)
    m = _fixture_ctx(g)
    gn = m.optimize(g["action"], g["obs1"], bw, 2)
    x2 = m.get_particles()
    _served(m, form, 1)
    m.close()
    errs = dict(disp_2=mpf_size_disp_err(x2, g), x_2=mpf_size_err(x2, g, "x_2"), grad_norms_2=mpf_size_err(gn, g, "grad_norms_2"))
    m = _fixture_ctx(g)
    gn = m.optimize(g["action"], g["obs1"], bw, n)
    errs.update(x_n=mpf_size_err(m.get_particles(), g, "x_n"), grad_norms=mpf_size_err(gn, g, "grad_norms"))
    gn = m.optimize(g["action2"], g["obs2"], bw, n)
    errs.update(x_n2=mpf_size_err(m.get_particles(), g, "x_n2"), grad_norms2=mpf_size_err(gn, g, "grad_norms2"))
    _served(m, form, 2)
    errs["probe_log_prob"] = mpf_size_err(m.prior_log_prob(g["probe"]), g, "probe_log_prob")
    m.close()
    print("%s [%s] " % (name, form) + "  ".join("%s %.1e/%.1e" % (q, e, float(g["tol_" + q])) for q, e in errs.items()))
    for q, e in errs.items():
        assert e < float(g["tol_" + q]), (name, form, q, e, float(g["tol_" + q]))


# ------------------------------------------------------------------------------------------------ size sweep against the oracle
SIZES = (1, 2, 7, 8, 63, 64, 65, 95, 96, 97, 255, 256, 257, 511, 512, 513, 1023, 1024)
SWEEP_MODELS = {
    # kind, uncertain, log space, bw, obs_std, past state, action, true (g, length, mass) or Particle mass
    "pend_lm": ("pendulum", ("length", "mass"), False, 0.15, 0.1, [3.0, 0.0], [1.3]),
    "pend_g3_log": ("pendulum", ("g", "length", "mass"), True, 0.35, 0.03, [1.5, 0.5], [1.3]),
    "part_log": ("particle", ("mass",), True, 0.5, 0.02, [-9.0, -9.0, 0.5, -0.25], [10.0, -14.0]),
}
SWEEP = [(mk, Mp, f) for mk in SWEEP_MODELS for Mp in SIZES for f in FORMS if f == "single" or Mp >= 8]


def _sweep_oracle(mk):
    from oracle import Oracle

    kind, up = SWEEP_MODELS[mk][:2]
    return Oracle(model=kind, uncertain_params=up, mass=2.0 if kind == "particle" else 1.0)


@functools.lru_cache(maxsize=None)
def _sweep_case(mk, Mp):
    """inputs of one sweep case and the oracle's answers (computed once, shared by the forms)"""
    from oracle import Oracle

    kind, up, ls, bw, std, past, act = SWEEP_MODELS[mk]
    rng = np.random.default_rng(1000 * len(mk) + Mp)
    P = len(up)
    if kind == "pendulum":
        centre = dict(g=9.8, length=1.0, mass=1.0)
        x0 = np.stack([centre[k] + (0.3 if k == "g" else 0.15) * rng.standard_normal(Mp) for k in up], 1).clip(min=0.3)
        truth = Oracle(model="pendulum", length=0.8, mass=1.25)
    else:
        x0 = (2.0 + 0.1 * rng.standard_normal((Mp, 1))).clip(min=0.5)
        truth = Oracle(model="particle", mass=3.0)
    x0 = (np.log(x0) if ls else x0).astype(np.float32)
    past, act = np.asarray(past, np.float32), np.asarray(act, np.float32)
    obs = truth.model_step(past[None], act[None])[0]
    # the repulsion term of phi is a sum over particles, not a mean: the step size shrinks with the particle count (the likelihood's
    # stiffness J^2 / obs_std^2 does not, hence the floor)
    lr = dict(pend_lm=0.02, pend_g3_log=0.01, part_log=0.1)[mk] / max(Mp, 16 if mk == "pend_lm" else 96)
    bwv = (bw * np.array([1.0, 1.3, 0.8])[:P]).astype(np.float32)  # P distinct prior bandwidths (the first prior of MPF(bw=None))
    o = _sweep_oracle(mk)
    ref = dict(x0=x0, past=past, act=act, obs=obs, lr=lr, bwv=bwv)
    ref["phi"] = o.mpf_phi(x0, x0, bw, past, act, obs, std, ls, bw)
    ref["phi_v"] = o.mpf_phi_v(x0, x0, bwv, past, act, obs, std, ls, bw)
    ref["x2"], _, _, ref["gn"] = o.mpf_optimize(x0, x0, bw, past, act, obs, std, ls, bw, lr, 2)
    ref["x2_v"], _, _, ref["gn_v"] = o.mpf_optimize_v(x0, x0, bwv, past, act, obs, std, ls, bw, lr, 2)
    return ref


def _disp_check(x2, x0, ref_x2, what):
    """two-step displacement by elemerr, at TOL scaled from position to displacement"""
    x0 = x0.astype(np.float64)
    want = ref_x2.astype(np.float64) - x0
    tol = TOL * _rms(ref_x2) / max(_rms(want), 1e-30)
    assert tol <= DISP_TOL_MAX, (what, tol)
    e = elemerr(x2.astype(np.float64) - x0, want)
    assert e < tol, (what, e, tol)
    assert elemerr(x2, ref_x2) < TOL, what
    return e, tol


@pytest.mark.parametrize("mk,Mp,form", SWEEP, ids=["%s-%d-%s" % c for c in SWEEP])
def test_size_sweep_vs_oracle(mk, Mp, form, monkeypatch):
    """Every edge of the launch geometry - one particle, one short of / exactly / one past a wave, the grid threshold (96), the KC = 4 / 8 /
    16 boundaries of the data-polled kernel (256 / 257, 512 / 513), the largest size and its ragged neighbour - for three models, in every
    eligible form: a two-step optimize() with a scalar and with P distinct prior bandwidths against Oracle.mpf_optimize(_v); in the
    one-workgroup form also the bare phi against Oracle.mpf_phi(_v)."""
    from dust_amd import MpfContext
    from oracle import grid_4x4_map

    kind, up, ls, bw, std, _, _ = SWEEP_MODELS[mk]
    r = _sweep_case(mk, Mp)
    _set_form(monkeypatch, form, Mp)
    kw = dict(model=kind, uncertain_params=up, log_space=ls, obs_std=std, lr=r["lr"], init_bw=bw, grid=grid_4x4_map() if kind == "particle" else None,
              mass=2.0 if kind == "particle" else 1.0)
    out = []
    for vec in ((False, True) if len(up) > 1 else (False,)):  # (P = 1: one bandwidth is the scalar case again)
        m = MpfContext(r["x0"], r["past"], **kw)
        if vec:
            m.set_prior_bw(r["bwv"])
        sfx = "_v" if vec else ""
        if form == "single":
            m.condition(r["act"], r["obs"])
            e = elemerr(m.phi(bw), r["phi" + sfx])
            assert e < TOL, ("phi" + sfx, e)
            gn = m.optimize(None, None, bw, 2)
        else:
            gn = m.optimize(r["act"], r["obs"], bw, 2)
        _served(m, form, 1)
        e_gn = elemerr(gn, r["gn" + sfx])
        assert e_gn < TOL, ("grad_norms" + sfx, e_gn)
        out.append(_disp_check(m.get_particles(), r["x0"], r["x2" + sfx], "displacement" + sfx) + (e_gn,))
        assert np.all(m.get_prior_bw() == np.float32(bw))  # update_prior(bw): isotropic again
        m.close()
    print("%s Mp %d [%s] " % (mk, Mp, form) + " | bw vector: ".join("disp %.1e/%.1e gn %.1e" % o for o in out))


# ------------------------------------------------------------------------------------------------ optimisers inside the grid forms
GRID_OPTIMS = [
    ("sgd_nesterov", torch.optim.SGD, dict(lr=2e-3, momentum=0.9, nesterov=True)),  # (lr is divided by the particle count below)
    ("rmsprop_centered_mom", torch.optim.RMSprop, dict(lr=1e-3, alpha=0.9, momentum=0.5, centered=True)),
    ("adagrad", torch.optim.Adagrad, dict(lr=2e-2, lr_decay=0.1, initial_accumulator_value=0.1)),
    ("adamw_amsgrad", torch.optim.AdamW, dict(lr=4e-3, betas=(0.9, 0.5), amsgrad=True, weight_decay=0.05)),  # (beta2 = 0.5: v falls where |phi| does, so max(v) != v)
]


@pytest.mark.parametrize("form", ("poll", "counter"))
@pytest.mark.parametrize("Mp", (130, 300, 600))
@pytest.mark.parametrize("oid,cls,opt", GRID_OPTIMS, ids=[c[0] for c in GRID_OPTIMS])
def test_grid_optimisers_follow_torch(oid, cls, opt, Mp, form, monkeypatch):
    """opt_step with the state slots opt_s0..opt_s2 inside the grid kernels: four two-step calls (state and step count persist across
    calls), each against a host loop from the same particles - phi from the CPU oracle, the step from the real torch.optim class,
    whose state is kept for the whole run.

    Bound: the two-step displacement tolerance, TOL * rms(x) / rms(displacement), NOT the 4 ulps of
    test_gpu_optim.py::test_mpf_steps_follow_torch_and_persist.  That test reads the device's own phi (dust_mpf_phi runs the one-workgroup
    kernel, as its optimize() does), so both sides see the same bits and only the update arithmetic differs.  A grid form sums phi in
    another order than dust_mpf_phi, and the second step of a call starts from the first, so its phi cannot be read from outside: the
    host's phi is the oracle's, equal to the device's to TOL, and the step inherits that.  The tolerance itself is capped (DISP_TOL_MAX).

    What this pins: the wiring of opt_step and its state slots in the grid kernels (which slot, which step count, carried across calls).
    RMSprop, Adagrad and AdamW normalise the step, so they say little about the SCALE of phi - the fixtures and the sweep hold phi."""
    from dust_amd import MpfContext
    from dust_amd.optim import optimizer_config
    from oracle import Oracle

    opt = dict(opt)
    if cls is torch.optim.SGD:
        opt["lr"] = opt["lr"] / Mp  # (the only one here whose step scales with phi, which grows with the particle count)
    rng = np.random.default_rng(Mp)
    x0 = (1.0 + 0.15 * rng.standard_normal((Mp, 2))).clip(min=0.3).astype(np.float32)
    bw, std = 0.15, 0.1
    past, act, obs = np.array([3.0, 0.0], np.float32), np.array([0.5], np.float32), np.array([2.9, -0.4], np.float32)
    _set_form(monkeypatch, form, Mp)
    m = MpfContext(x0, past, model="pendulum", uncertain_params=("length", "mass"), obs_std=std, init_bw=bw, lr=float(opt["lr"]),
                   optim=optimizer_config(cls, opt))
    m.condition(act, obs)
    o = Oracle(model="pendulum", uncertain_params=("length", "mass"))
    p = torch.tensor(x0.copy(), requires_grad=True)
    host = cls([p], **opt)
    worst, worst_tol = 0.0, 0.0
    for call in range(4):
        before = m.get_particles()
        m.optimize(None, None, bw, 2)
        after = m.get_particles()
        with torch.no_grad():
            p.copy_(torch.from_numpy(before))  # (every call is a first-divergence comparison; the optimiser's state is the host's own)
        for _ in range(2):
            x = p.detach().numpy().copy()
            p.grad = torch.from_numpy(-o.mpf_phi(x, x, bw, past, act, obs, std, False, bw))  # (the prior's means alias the particles)
            host.step()
        want = p.detach().numpy().astype(np.float64) - before
        tol = TOL * _rms(after) / _rms(want)
        assert tol <= DISP_TOL_MAX, (oid, Mp, call, tol)  # (the optimiser moved the particles: steps are compared, not rounding)
        e = elemerr(after.astype(np.float64) - before, want)
        worst, worst_tol = max(worst, e / tol), max(worst_tol, tol)
        assert e < tol, (oid, Mp, form, call, e, tol)
    _served(m, form, 4)
    m.close()
    st = host.state[p]
    if "max_exp_avg_sq" in st:  # AMSGrad: the max slot must differ from v somewhere, or the slot is not exercised
        assert float((st["max_exp_avg_sq"] > 1.01 * st["exp_avg_sq"]).float().mean()) > 0.1
    print("%s Mp %d [%s]: worst displacement error / tolerance %.2f, largest tolerance %.1e" % (oid, Mp, form, worst, worst_tol))


# ------------------------------------------------------------------------------------------------ the prior's density
@pytest.mark.parametrize("P", (1, 2, 3))
@pytest.mark.parametrize("K", (1, 65, 1024))
def test_prior_log_prob_vs_float64(K, P):
    """dust_mpf_prior_log_prob: a K-component Gaussian mixture over P dimensions with per-dimension bandwidths, at a probe count that is
    not a multiple of the block size (256), probes 40 bandwidths away from EVERY mean included (every exponent is below -800: a sum of
    bare exponentials is 0 there), against a float64 log-sum-exp.

    Metric: |got - want| / (|want| + 1) per probe, not helpers.elemerr.  The values span 1 ... 3 000 here (the far probes), so elemerr's
    rms floor would be ~1e2 and hide an error on a probe near a component, whose log-density is of order 1; the floor 1 is tighter for
    those and the same for the far ones."""
    from dust_amd import MpfContext

    up = (("mass",), ("length", "mass"), ("g", "length", "mass"))[P - 1]
    rng = np.random.default_rng(100 * K + P)
    centre = np.array([9.8, 1.0, 1.0])[3 - P:]
    means = (centre + 0.2 * rng.standard_normal((K, P))).astype(np.float32)
    bwv = np.array([0.11, 0.07, 0.19], np.float32)[:P]
    n = 517
    probes = (centre + 0.3 * rng.standard_normal((n, P))).astype(np.float32)
    probes[:64] = means[rng.integers(0, K, 64)] + (0.5 * bwv * rng.standard_normal((64, P))).astype(np.float32)  # close to a component
    far = means.max(0) + 40.0 * bwv  # >= 40 bandwidths from every mean in every dimension
    probes[-5:] = far + np.abs(rng.standard_normal((5, P))).astype(np.float32) * bwv
    probes[-6] = means.min(0) - 41.0 * bwv  # (41: the fp32 rounding of the probe must not bring it inside 40)
    m = MpfContext(means, np.array([3.0, 0.0], np.float32), model="pendulum", uncertain_params=up, init_bw=float(bwv[0]))
    m.set_prior_bw(bwv)
    got = m.prior_log_prob(probes)
    m.close()
    z = (probes.astype(np.float64)[:, None, :] - means.astype(np.float64)[None]) / bwv.astype(np.float64)
    e = -0.5 * (z * z).sum(-1)
    assert np.all(e[-6:].max(1) < -800.0 * P)
    mx = e.max(1, keepdims=True)
    want = (mx[:, 0] + np.log(np.exp(e - mx).sum(1)) - np.log(K) - np.log(bwv.astype(np.float64)).sum() - 0.5 * P * np.log(2.0 * np.pi))
    assert np.isfinite(got).all()
    err = float((np.abs(got - want) / (np.abs(want) + 1.0)).max())  # relative to each value's own size (values of order 1 ... 1e3)
    assert err < TOL, (K, P, err)
