"""The dynamics filter on the skid-steer robot (mpf.hpp mpf_skid_score, skid.hpp skid_step_cs) against the reference's own MPF +
GaussianLikelihood on its SkidSteerRobot (tests/golden/mpf_skid_*.npz, made by tests/golden/make_golden_mpf_skid.py; the scenarios are
data in tests/mpf_skid_cases.py).  The oracle has no skid-steer filter: the reference fixtures are the independent side.

As in test_gpu_mpf_sizes.py the three forms of the optimisation kernel (single / poll / counter) are selected by the development
switches and asserted through stats(); tolerances are the fixtures' own, measured from the reference alone; two-step calls are
compared by displacement.
"""
import copy
import ctypes as C

import numpy as np
import pytest
import torch

from helpers import elemerr, mpf_size_disp_err, mpf_size_err
from mpf_skid_cases import BY_TAG, NAMES, NAMES3, SWEEP_SIZES, TRUE, model_kwargs, particles, sweep_scenario
from test_gpu_mpf_sizes import FORMS, _served, _set_form

pytestmark = pytest.mark.gpu


def _ctx(s, x0, obs0, **kw):
    from dust_amd import MpfContext

    return MpfContext(x0, obs0, lr=s["lr"], init_bw=s["bw"], optimizer=s["opt"], **model_kwargs(s), **kw)


# ------------------------------------------------------------------------------------------------ fixtures x forms
@pytest.mark.parametrize("name", NAMES)
def test_fixture_phi_vs_reference(golden, name):
    """dust_mpf_phi against the reference's MPF.phi; the fixture's power: with its branch ignored the reference itself is >= 10
    tolerances away."""
    g, s = golden("mpf_skid_" + name), BY_TAG[name]
    m = _ctx(s, g["x0"], g["obs0"])
    m.condition(g["action"], g["obs1"])
    phi = m.phi(float(g["bw"]))
    e = mpf_size_err(phi, g, "phi0")
    print("%s phi0: err %.2e tol %.2e" % (name, e, float(g["tol_phi0"])))
    assert e < float(g["tol_phi0"])
    off = g["phi0_off"]
    assert elemerr(off, g["phi0"][:off.shape[0]]) >= 10 * float(g["tol_phi0"])
    assert elemerr(off, phi[:off.shape[0]]) >= 9 * float(g["tol_phi0"])  # (and so is the device)
    assert np.array_equal(m.get_particles(), g["x0"])
    m.close()


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("name", NAMES)
def test_fixture_optimize_vs_reference(golden, name, form, monkeypatch):
    """A two-step optimize() and two full calls (optimiser state carried over), in every form, against the reference's MPF.optimize;
    then the resulting prior's log-density."""
    g, s = golden("mpf_skid_" + name), BY_TAG[name]
    Mp, bw, n = int(g["Mp"]), float(g["bw"]), int(g["n_steps"])
    _set_form(monkeypatch, form, Mp)
    m = _ctx(s, g["x0"], g["obs0"])
    gn = m.optimize(g["action"], g["obs1"], bw, 2)
    x2 = m.get_particles()
    _served(m, form, 1)
    m.close()
    errs = dict(disp_2=mpf_size_disp_err(x2, g), x_2=mpf_size_err(x2, g, "x_2"), grad_norms_2=mpf_size_err(gn, g, "grad_norms_2"))
    m = _ctx(s, g["x0"], g["obs0"])
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


# ------------------------------------------------------------------------------------------------ the size sweep x forms
SWEEP = [(Mp, f) for Mp in SWEEP_SIZES for f in FORMS if f == "single" or Mp >= 8]


@pytest.mark.parametrize("Mp,form", SWEEP, ids=["%d-%s" % c for c in SWEEP])
def test_size_sweep_vs_reference(golden, Mp, form, monkeypatch):
    """P = 3 in log space at every edge of the launch geometry (one particle, around a wave, the grid threshold, the KC boundaries of the
    data-polled kernel, the largest size and its ragged neighbour): a two-step optimize() in every eligible form - and the bare phi in
    the one-workgroup form - against the reference, x0 rebuilt from the seeded function the generator used."""
    g, s = golden("mpf_skid_sweep"), sweep_scenario(Mp)
    x0 = particles(s["up"], Mp, s["log"], s["seed"], s["spread"])
    q = lambda k: g["%s_%d" % (k, Mp)]
    _set_form(monkeypatch, form, Mp)
    m = _ctx(s, x0, g["obs0"])
    if form == "single":
        m.condition(g["action"], g["obs1"])
        phi = m.phi(s["bw"])
        e = min(elemerr(phi, q("phi0")), elemerr(phi, q("phi0_f64")))
        assert e < float(q("tol_phi0")), ("phi0", e, float(q("tol_phi0")))
        gn = m.optimize(None, None, s["bw"], 2)
    else:
        gn = m.optimize(g["action"], g["obs1"], s["bw"], 2)
    x2 = m.get_particles()
    _served(m, form, 1)
    m.close()
    e_gn = min(elemerr(gn, q("grad_norms_2")), elemerr(gn, q("grad_norms_2_f64")))
    d = x2.astype(np.float64) - x0
    e_d = min(elemerr(d, q("x_2").astype(np.float64) - x0), elemerr(d, q("disp_2_f64")))
    e_x = min(elemerr(x2, q("x_2")), elemerr(x2, x0.astype(np.float64) + q("disp_2_f64")))
    print("Mp %d [%s] disp %.1e/%.1e  x_2 %.1e/%.1e  gn %.1e/%.1e" % (Mp, form, e_d, float(q("tol_disp_2")), e_x, float(q("tol_x_2")), e_gn,
                                                                     float(q("tol_grad_norms_2"))))
    assert e_gn < float(q("tol_grad_norms_2")) and e_d < float(q("tol_disp_2")) and e_x < float(q("tol_x_2"))


# ------------------------------------------------------------------------------------------------ the dual tick
def _plant(st, a, dt=0.1):
    """SkidSteerRobot.step with the plant's parameters (any plant does: both sides of a comparison see the same states)"""
    r, l = np.clip(a, -0.5, 0.5).astype(np.float64)
    lin = (r + l) * np.pi * TRUE["wheel_radius"]
    ang = (r - l) * 2 * np.pi * TRUE["wheel_radius"] / TRUE["axial_distance"]
    fwd, lat = lin * dt, -ang * TRUE["x_icr"] * dt
    c, s = np.cos(st[2]), np.sin(st[2])
    return np.array([st[0] + fwd * c - lat * s, st[1] + fwd * s + lat * c, st[2] + ang * dt, lin, ang], np.float32)


def test_dual_tick_on_skid_steer_equals_its_pieces():
    """dust_dual_tick with a skid-steer controller and filter that name the same uncertain parameters: the filter update with Silverman's
    bandwidth on the device, the controller's dynamics samples drawn from the refreshed prior on the device, the control tick - one call
    - against the same pieces called one by one with the same Philox key: bit-identical over three control periods.  A controller that
    names other parameters than the filter is refused."""
    from dust_amd import Context, MpfContext, _lib

    N, S, M, H, K, Mp = 32, 16, 3, 8, 2, 130
    rng = np.random.default_rng(11)
    mu = (0.2 * rng.standard_normal((N, H, 2))).astype(np.float32)
    th = (mu + 0.1 * rng.standard_normal((N, H, 2))).astype(np.float32)
    x0 = particles(NAMES3, Mp, True, 77, 0.2)
    s0 = np.array([0.3, -0.2, 0.7, 0.0, 0.0], np.float32)
    goal = (1.0, 0.5, 0.0, 0.0, 0.0)

    def make(up=NAMES3):
        c = Context(model="skid_steer", N=N, S=S, M=M, H=H, dt=0.1, kernel="K1", lr=0.05, alpha=0.5, sigma_a=0.3, sigma_p=0.3, uncertain_params=up,
                    params_log_space=True, goal=goal, w_quad_ctrl=(0.1, 0.1), seed=5)
        c.set_theta(th); c.set_prior(mu); c.set_a_mat(th)
        m = MpfContext(x0, s0, model="skid_steer", uncertain_params=NAMES3, log_space=True, obs_std=0.05, lr=1e-4, init_bw=0.3, dt=0.1)
        return c, m

    ca, ma = make()
    cb, mb = make()
    sa = sb = s0
    prev = None
    for t in range(3):
        a1, p1, bw1 = ca.dual_tick(ma, sa, prev, K, mpf_steps=6, mpf_bw=None, seed=100 + t)
        if prev is not None:
            bw2 = mb.silverman()
            mb.optimize(prev, sb, bw2, 6)
            assert bw1 == bw2
        params = mb.prior_sample(K * M, 100 + t).reshape(K, M, 3)
        a2, p2 = cb.svmpc_tick(sb, K, None, params)
        assert np.isfinite(a1).all() and abs(float(p1.sum()) - 1.0) < 1e-4
        assert np.array_equal(a1, a2) and np.array_equal(p1, p2), t
        assert np.array_equal(ma.get_particles(), mb.get_particles()), t
        prev = a1[0].copy()
        sa = sb = _plant(sa, a1[0])
    assert np.array_equal(ca.get_theta(), cb.get_theta())
    assert ma.stats() == mb.stats() == {"grid": 2, "fallback": 0}  # (130 particles, 6 steps: the data-polled grid ran the updates)
    assert not np.array_equal(ma.get_particles(), x0)
    cw = Context(model="skid_steer", N=N, S=S, M=M, H=H, dt=0.1, kernel="K1", uncertain_params=NAMES3[::-1], params_log_space=True, goal=goal)
    with pytest.raises(_lib.DustError) as e:
        cw.dual_tick(ma, sa, None, K)
    assert e.value.status == _lib.ERR_INVALID
    for o in (ca, cb, cw, ma, mb):
        o.close()


# ------------------------------------------------------------------------------------------------ the mirror classes
@pytest.mark.parametrize("name", ("p3_log", "nondefault"))
def test_mirror_mpf_over_skid_steer_reproduces_the_fixture(golden, name):
    """MPF(init, GaussianLikelihood(obs, std, SkidSteerRobot(...), log_space)): params_dict, uncertain_params, the action space's bounds
    and dt reach the device from the model object."""
    from dust_amd.inference import MPF, GaussianLikelihood
    from dust_amd.models import SkidSteerRobot

    g, s = golden("mpf_skid_" + name), BY_TAG[name]
    model = SkidSteerRobot(delta_t=s["dt"], min_wheel_speed=torch.tensor(s["lo"]), max_wheel_speed=torch.tensor(s["hi"]), uncertain_params=s["up"],
                           **s["fixed"])
    lik = GaussianLikelihood(torch.tensor(g["obs0"]), s["obs_std"], model, log_space=s["log"])
    mpf = MPF(torch.tensor(g["x0"]), lik, bw=s["bw"], bw_scale=1.0, optimizer_class=torch.optim.SGD, lr=s["lr"])
    lik.condition(torch.tensor(g["action"]).view(1, 2), torch.tensor(g["obs1"]))
    mpf._dev.condition(g["action"], g["obs1"])
    assert mpf_size_err(mpf.phi(s["bw"]).numpy(), g, "phi0") < float(g["tol_phi0"])
    mpf = MPF(torch.tensor(g["x0"]), GaussianLikelihood(torch.tensor(g["obs0"]), s["obs_std"], model, log_space=s["log"]), bw=s["bw"], bw_scale=1.0,
              optimizer_class=torch.optim.SGD, lr=s["lr"])
    gn, bw = mpf.optimize(torch.tensor(g["action"]).view(1, 2), torch.tensor(g["obs1"]), bw=s["bw"], n_steps=s["n"])
    assert bw == s["bw"]
    assert mpf_size_err(mpf.x.numpy(), g, "x_n") < float(g["tol_x_n"])
    assert mpf_size_err(gn.numpy(), g, "grad_norms") < float(g["tol_grad_norms"])
    twin = copy.deepcopy(mpf)  # (dust_mpf_clone copies the model)
    gn, _ = mpf.optimize(torch.tensor(g["action2"]).view(1, 2), torch.tensor(g["obs2"]), bw=s["bw"], n_steps=s["n"])
    gt, _ = twin.optimize(torch.tensor(g["action2"]).view(1, 2), torch.tensor(g["obs2"]), bw=s["bw"], n_steps=s["n"])
    assert mpf_size_err(mpf.x.numpy(), g, "x_n2") < float(g["tol_x_n2"])
    assert mpf_size_err(gn.numpy(), g, "grad_norms2") < float(g["tol_grad_norms2"])
    assert torch.equal(mpf.x, twin.x) and torch.equal(gn, gt)
    assert mpf_size_err(mpf.prior.log_prob(torch.tensor(g["probe"])).numpy(), g, "probe_log_prob") < float(g["tol_probe_log_prob"])


def test_dual_svmpc_on_skid_steer_fused_equals_unfused():
    """DualSVMPC over SkidSteerRobot, five control periods: fused (one C call per period) and unfused (the loop's own calls) give the
    same actions, weights and filter particles.  An explicit filter bandwidth and one SVGD iteration per tick, so that both draw the same
    dynamics samples (the unfused loop draws one set per iteration and evaluates Silverman's rule on the host)."""
    from dust_amd.controllers import DualSVMPC, MultiDISCO
    from dust_amd.costs import QuadraticCost
    from dust_amd.inference import MPF, SVMPC, ExponentiatedUtility, GaussianLikelihood, get_gmm
    from dust_amd.kernels import RBFKernel
    from dust_amd.models import SkidSteerRobot

    N, S, M, H, Mp = 16, 16, 3, 6, 130
    rng = np.random.default_rng(21)
    mu0 = torch.tensor((0.2 * rng.standard_normal((N, H, 2))).astype(np.float32))
    init_policies = mu0 + torch.tensor((0.1 * rng.standard_normal((N, H, 2))).astype(np.float32))
    x0 = torch.tensor(particles(NAMES3, Mp, True, 78, 0.2))
    init_state = torch.tensor([0.3, -0.2, 0.7, 0.0, 0.0])
    cost = QuadraticCost((1.0, 0.5, 0.0, 0.0, 0.0), (1, 1, 1, 1, 1), (1, 1, 1, 1, 1), (0.1, 0.1))

    def make(fused):
        model = SkidSteerRobot(delta_t=0.1, uncertain_params=NAMES3)
        ctrl = MultiDISCO(observation_space=model.observation_space, action_space=model.action_space, hz_len=H, action_samples=S, params_samples=M,
                          temperature=2.0, a_cov=0.09 * torch.eye(2), inst_cost_fn=cost.inst_cost, term_cost_fn=cost.term_cost, params_sampling=True,
                          n_policies=N, params_log_space=True, seed=5)
        ctrl.a_mat = init_policies.clone()
        ctrl.return_rollouts = False
        mpf = MPF(init_particles=x0.clone(), likelihood=GaussianLikelihood(initial_obs=init_state, obs_std=0.05, model=model, log_space=True),
                  optimizer_class=torch.optim.SGD, lr=1e-4, bw=0.3, bw_scale=1.0)
        sv = SVMPC(likelihood=ExponentiatedUtility(alpha=0.5, n_samples=S, controller=ctrl, model=model), init_particles=init_policies.clone(),
                   prior=get_gmm(mu0, torch.ones(N), 0.09 * torch.eye(2)), kernel=RBFKernel(), n_particles=N, bw_scale=1.0, n_steps=1,
                   optimizer_class=torch.optim.SGD, lr=0.05)
        return DualSVMPC(sv, mpf, mpf_bw=0.3, mpf_steps=6, warm_up=0, fused=fused, seed=0)

    def plant(state, action):
        return torch.from_numpy(_plant(state.reshape(-1).numpy(), action.reshape(-1).numpy())).reshape(1, -1)

    fu, un = make(True), make(False)
    sf = su = init_state.reshape(1, -1)
    for t in range(5):
        af, sf, pf = fu.tick(sf, plant)
        au, su, pu = un.tick(su, plant)
        assert torch.isfinite(af).all() and abs(float(pf.sum()) - 1.0) < 1e-4, t
        assert torch.equal(af, au) and torch.equal(pf, pu) and torch.equal(sf, su), t
    assert fu._pending is not None and un._pending is None  # (the fused loop carries its last filter update out when the filter is read)
    assert torch.equal(fu.dyn_particles, un.dyn_particles) and not torch.equal(un.dyn_particles, x0)
    assert torch.equal(fu.theta, un.theta)


# ------------------------------------------------------------------------------------------------ refusals
def _raw_create(P=3, ctrl_noise=0):
    """dust_mpf_create for the skid-steer model WITHOUT the dust_mpf_set_skid_steer call MpfContext adds; (status, handle)"""
    from dust_amd import _lib as L
    from dust_amd.backend import make_config

    c = L.MpfConfig()
    c.abi_version, c.device, c.n_particles, c.dim_p = L.ABI_VERSION, 0, 16, P
    c.model_cfg = make_config(model="skid_steer", uncertain_params=NAMES3[:P], dt=0.1)
    c.model_cfg.ctrl_noise = ctrl_noise
    c.dim_s, c.dim_a, c.model = 5, 2, L.MODEL_SKID_STEER
    c.log_space, c.obs_std, c.lr, c.bw_scale, c.init_bw = 0, 0.05, 1e-6, 1.0, 0.05
    x = particles(NAMES3[:P], 16, False, 5, 0.15)
    obs = np.zeros(5, np.float32)
    h = L.VP()
    st = L.load().dust_mpf_create(C.byref(c), x.ctypes.data_as(L.FP), obs.ctypes.data_as(L.FP), C.byref(h))
    return st, h


def test_refusals():
    from dust_amd import MpfContext, _lib as L

    lib = L.load()
    st, h = _raw_create(ctrl_noise=1)  # ctrl_noise stays a Particle field
    assert st == L.ERR_UNSUPPORTED and not h.value
    st, h = _raw_create()
    assert st == L.OK
    act, obs, phi = np.array([0.4, -0.25], np.float32), np.full(5, 0.01, np.float32), np.empty((16, 3), np.float32)
    assert lib.dust_mpf_condition(h, act.ctypes.data_as(L.FP), obs.ctypes.data_as(L.FP)) == L.OK
    # before dust_mpf_set_skid_steer nothing is sampled: phi and optimize have no column to differentiate
    assert lib.dust_mpf_phi(h, 0.05, phi.ctypes.data_as(L.FP)) == L.ERR_STATE
    assert lib.dust_mpf_optimize(h, None, None, 0.05, 2, None) == L.ERR_STATE
    g = L.SkidConfig()
    g.x_icr, g.wheel_radius, g.axial_distance = L.Param(L.PARAM_SAMPLED, 0, 0.2), L.Param(L.PARAM_SAMPLED, 1, 0.0625), L.Param(L.PARAM_PYFLOAT, 0, 0.475)
    for d in range(2):
        g.min_wheel_speed[d], g.max_wheel_speed[d] = -0.5, 0.5
    assert lib.dust_mpf_set_skid_steer(h, C.byref(g)) == L.OK
    assert lib.dust_mpf_phi(h, 0.05, phi.ctypes.data_as(L.FP)) == L.ERR_STATE  # two sampled columns do not cover dim_p = 3
    g.axial_distance = L.Param(L.PARAM_SAMPLED, 3, 0.475)
    assert lib.dust_mpf_set_skid_steer(h, C.byref(g)) == L.ERR_INVALID  # a sampled column outside dim_p
    g.axial_distance = L.Param(L.PARAM_SAMPLED, 1, 0.475)
    assert lib.dust_mpf_set_skid_steer(h, C.byref(g)) == L.ERR_INVALID  # a column named twice
    g.axial_distance = L.Param(L.PARAM_SAMPLED, 2, 0.475)
    g.min_wheel_speed[0] = 0.6
    assert lib.dust_mpf_set_skid_steer(h, C.byref(g)) == L.ERR_INVALID  # min > max
    g.min_wheel_speed[0] = -0.5
    assert lib.dust_mpf_set_skid_steer(h, C.byref(g)) == L.OK
    assert lib.dust_mpf_phi(h, 0.05, phi.ctypes.data_as(L.FP)) == L.OK and np.isfinite(phi).all()
    lib.dust_mpf_destroy(h)
    # through the wrapper: a P = 1 filter cannot take two sampled parameters
    m = MpfContext(particles(("axial_distance",), 16, False, 5, 0.15), np.zeros(5, np.float32), model="skid_steer", uncertain_params=("axial_distance",), dt=0.1)
    with pytest.raises(L.DustError) as e:
        m.set_skid_steer(uncertain_params=("x_icr", "wheel_radius"))
    assert e.value.status == L.ERR_INVALID
    m.close()
    with pytest.raises(L.DustError) as e:  # the pendulum's filter has no skid-steer model to set
        p = MpfContext(np.ones((4, 2), np.float32), np.array([3.0, 0.0], np.float32))
        p.set_skid_steer(uncertain_params=("x_icr", "wheel_radius"))
    assert e.value.status == L.ERR_STATE
    p.close()
