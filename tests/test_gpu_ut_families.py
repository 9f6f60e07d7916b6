"""Sigma-point rollouts ("DISCO" case: MultiDISCO(params_sampling=MerweScaledUTF), disco.py:211-292, 312-323) of the skid-steer and cart-pole
families, the sigma points of the filter's prior on the device (dust_mpf_sigma_points) and the fused dual tick over a sigma-point
controller, against the reference's own numbers (tests/golden/make_golden_ut_families.py; scenarios in tests/ut_cases.py).  Every bound
is the fixture's stored tolerance - measured from the reference alone - except omega / a_mix, which carry the cost-ulp amplification of
test_unscented_transform_disco_vs_reference, and params_log_p at 1e-5."""
import copy

import numpy as np
import pytest
import torch

import cartpole_cases as cpc
from helpers import elemerr, relerr
from ut_cases import (FAMILY, ROLLOUT_BY_TAG, ROLLOUT_NAMES, SIGMA_BY_TAG, SIGMA_NAMES, SIGMA_UP, TICK_BY_TAG, TICK_NAMES, context_kwargs, twin,
                      weights)

pytestmark = pytest.mark.gpu
TOL = 1e-5


def _err(got, g, q):
    """elemerr against the reference's fp32 or float64 value of quantity q, whichever is nearer"""
    return min(elemerr(got, g[q]), elemerr(got, twin(g, q)))


def _ctx(s, **kw):
    from dust_amd import Context

    return Context(**context_kwargs(s, **kw))


def _mirror_model(s):
    from dust_amd.models import CartPoleModel, SkidSteerRobot

    f = FAMILY[s["family"]]
    if s["family"] == "cartpole":
        return CartPoleModel(dt=f["dt"], uncertain_params=s["up"], **f["defaults"])
    return SkidSteerRobot(delta_t=f["dt"], min_wheel_speed=torch.tensor(f["lo"]), max_wheel_speed=torch.tensor(f["hi"]), uncertain_params=s["up"],
                          **f["defaults"])


def _mirror_controller(s, model, alpha_ut, **kw):
    from dust_amd.controllers import MultiDISCO
    from dust_amd.costs import QuadraticCost
    from dust_amd.utils.utf import MerweScaledUTF

    f = FAMILY[s["family"]]
    cost = QuadraticCost(f["goal"], f["w_state"], f["w_term"])  # (no control weight: the sigma-point mode's instantaneous cost is action-free)
    return MultiDISCO(observation_space=model.observation_space, action_space=model.action_space, hz_len=s["H"], n_policies=s["N"],
                      action_samples=s["S"], temperature=f["temperature"], a_cov=f["sigma_a"] ** 2 * torch.eye(f["da"]), inst_cost_fn=cost.inst_cost,
                      term_cost_fn=cost.term_cost, params_sampling=MerweScaledUTF(n=len(s["up"]), alpha=alpha_ut, **kw), params_log_space=False)


def _dist(g):
    return torch.distributions.MultivariateNormal(torch.tensor(g["dist_mean"]), covariance_matrix=torch.diag(torch.tensor(g["dist_std"]) ** 2))


# ------------------------------------------------------------------------------------------------ 1. rollouts
@pytest.mark.parametrize("via", ["context", "mirror"])
@pytest.mark.parametrize("name", ROLLOUT_NAMES)
def test_sigma_point_rollouts_vs_reference(golden, name, via):
    """The family's first-pass kernel in its sigma-point form + the regular kernel's weights stage on the injected costs, against the
    reference's MultiDISCO.forward: through the raw Context (set_param_weights, the sigma points as params) and through the mirror."""
    g, s = golden("ut_" + name), ROLLOUT_BY_TAG[name]
    f = FAMILY[s["family"]]
    if via == "context":
        c = _ctx(s)
        c.set_param_weights(g["loc_weights"])
        c.set_a_mat(g["a_mat0"])
        costs, states, _, omega = c.disco_forward(g["state"], g["ext_actions"], params=g["sigma_points"], want_states=True)
        got = dict(costs=costs, states=states, omega=omega, a_mat1=c.get_a_mat(), a_mix=c.get_a_mix())
        c.close()
    else:
        from dust_amd.utils.utf import MerweScaledUTF

        model = _mirror_model(s)
        ctrl = _mirror_controller(s, model, float(g["alpha"]))
        assert ctrl.n_params == 1  # disco.py:128: the sigma points are internal to the rollouts
        ctrl.a_mat = torch.tensor(g["a_mat0"])
        costs, states, _, omega, plp = ctrl.forward(torch.tensor(g["state"]), model, _dist(g), ext_actions=torch.tensor(g["ext_actions"]))
        got = dict(costs=costs.numpy(), states=states.numpy(), omega=omega.numpy(), a_mat1=ctrl.a_mat.numpy(), a_mix=ctrl.a_mix.numpy())
        assert relerr(plp.numpy(), g["params_log_p"]) < 1e-5
        tf = MerweScaledUTF(n=len(s["up"]), alpha=float(g["alpha"]))
        assert relerr(tf.compute_sigma_points(torch.tensor(g["dist_mean"]), torch.diag(torch.tensor(g["dist_std"]) ** 2)).T.numpy(), g["sigma_points"]) < 1e-6
    quant = ("costs", "a_mat1") + (("states",) if s["states"] else ())
    errs = {q: (_err(got[q], g, q), float(g["tol_" + q])) for q in quant}
    assert got["states"].shape == (int(g["M"]), s["S"], s["N"], s["H"] + 1, f["ds"]) and np.isfinite(got["states"]).all()
    # the weights carry the amplification of one cost ulp through exp(-cost / temperature) (test_unscented_transform_disco_vs_reference)
    wtol = 8 * float(np.spacing(np.float32(np.abs(g["costs"]).max()))) / f["temperature"]
    for q in ("omega", "a_mix"):  # (against the reference's fp32 or float64 value, whichever is nearer, as every quantity here)
        errs[q] = (min(relerr(got[q], g[q]), relerr(got[q], g[q + "_f64"])), wtol)
    power = elemerr(got["costs"], g["costs_off"])
    print("%s [%s] " % (name, via) + "  ".join("%s %.1e/%.1e" % (q, e, t) for q, (e, t) in errs.items()) + "  power %.1e" % power)
    for q, (e, t) in errs.items():
        assert e < t, (name, via, q, e, t)
    assert power >= 5 * float(g["tol_costs"])  # the device is on the reference's side of the (sigma, step) weight pattern
    if "costs_mean" in g:
        assert elemerr(got["costs"], g["costs_mean"]) >= 5 * float(g["tol_costs"])


# ------------------------------------------------------------------------------------------------ 2. whole ticks
@pytest.mark.parametrize("name", TICK_NAMES)
def test_sigma_point_ticks_vs_reference(golden, name):
    """TICK_ITERS SVGD iterations (K1, SGD) and forward() of SVMPC over a sigma-point controller against the reference's: score and phi
    with the reference's costs and actions injected (svmpc_phi), then the mirror's SVMPC from the recorded policy noise - costs and
    particles per iteration, log_l, log_p, p_weights, the argmax, a_seq.  Device-drawn noise, step("average") and a deep copy: shapes
    and finiteness."""
    from dust_amd.inference import SVMPC, ExponentiatedUtility, get_gmm
    from dust_amd.kernels import RBFKernel

    g, s = golden("ut_" + name), TICK_BY_TAG[name]
    f = FAMILY[s["family"]]
    K, N, S, H = int(g["K"]), s["N"], s["S"], s["H"]
    mix = np.ones(N, np.float32)
    errs = {}
    c = _ctx(s, kernel="K1", optimizer="SGD", lr=s["lr"], alpha=s["alpha"])
    c.set_param_weights(g["loc_weights"])
    for k in range(K):
        c.set_theta(g["theta_in"][k])
        c.set_prior(g["mu0"], mix)
        phi, gl, gp = c.svmpc_phi(g["costs"][k], g["actions"][k])
        for q, v in (("score", gl + gp), ("phi", phi)):
            errs["%s[%d]" % (q, k)] = (min(elemerr(v, g[q][k]), elemerr(v, g[q + "_f64"][k])), float(g["tol_" + q]))
    c.close()
    model = _mirror_model(s)
    ctrl = _mirror_controller(s, model, float(g["alpha_ut"]))
    ctrl.a_mat = torch.tensor(g["theta0"])
    ctrl.return_rollouts = False
    cov = f["sigma_a"] ** 2 * torch.eye(f["da"])
    lik = ExponentiatedUtility(alpha=s["alpha"], n_samples=S, controller=ctrl, model=model)
    sv = SVMPC(likelihood=lik, init_particles=torch.tensor(g["theta0"]), prior=get_gmm(torch.tensor(g["mu0"]), torch.ones(N), cov), kernel=RBFKernel(),
               n_particles=N, bw_scale=1.0, n_steps=1, optimizer_class=torch.optim.SGD, lr=s["lr"])
    pd, state = _dist(g), torch.tensor(g["state"])
    for k in range(K):
        sv.optimize(state, pd, n_steps=1, eps=g["eps"][k][None])
        for q, v in (("costs", sv._ctx().get_costs()), ("theta_after", sv.theta.numpy())):
            errs["%s[%d]" % (q, k)] = (min(elemerr(v, g[q][k]), elemerr(v, g[q + "_f64"][k])), float(g["tol_" + q]))
    a_seq, pw = sv.forward(state, pd)
    ll, lp = sv._ctx().get_log_weights()
    for q, v in (("log_l", ll), ("log_p", lp), ("p_weights", pw.numpy())):
        errs[q] = (_err(v, g, q), float(g["tol_" + q]))
    errs["a_seq"] = (elemerr(a_seq.numpy(), g["a_seq"]), float(g["tol_theta_after"]))  # (a row of the particles the chain above led to)
    assert int(np.argmax(pw.numpy())) == int(np.argmax(g["p_weights"]))
    print(name + " " + "  ".join("%s %.1e/%.1e" % (q, e, t) for q, (e, t) in errs.items()))
    for q, (e, t) in errs.items():
        assert e < t, (name, q, e, t)
    # the controller's own noise, step("average"), a deep copy: the draws differ from torch's
    sv.optimize(state, pd, n_steps=1)
    a_seq, pw = sv.forward(state, pd)
    assert a_seq.shape == (H, f["da"]) and torch.isfinite(a_seq).all() and abs(float(pw.sum()) - 1.0) < 1e-4
    ctrl.forward(state, model, pd)
    a = ctrl.step(strategy="average")
    assert a.shape == (1, f["da"]) and torch.isfinite(a).all()
    c2 = copy.deepcopy(ctrl)  # (the weights and the scale travel with the clone)
    c3 = c2.forward(state, model, pd)[0]
    assert c3.shape == (S, N) and torch.isfinite(c3).all()


# ------------------------------------------------------------------------------------------------ 3. the plain path
@pytest.mark.parametrize("name", ["cartpole_p2", "skid_p2"])
def test_clearing_the_weights_restores_the_plain_costs_bit_for_bit(golden, name):
    g, s = golden("ut_" + name), ROLLOUT_BY_TAG[name]
    c = _ctx(s)

    def costs():
        c.set_a_mat(g["a_mat0"])
        return c.disco_forward(g["state"], g["ext_actions"], params=g["sigma_points"])[0].copy()

    plain = costs()
    assert elemerr(plain, g["costs_mean"]) < float(g["tol_costs"])  # (without weights: the mean over the five parameter rows)
    c.set_param_weights(g["loc_weights"])
    c.set_sigma_scale(float(g["sigma_scale"]))
    assert _err(costs(), g, "costs") < float(g["tol_costs"])
    c.set_param_weights(None)
    assert np.array_equal(costs(), plain)
    c.close()


# ------------------------------------------------------------------------------------------------ 4. refusals
@pytest.mark.parametrize("name", ["cartpole_p1", "skid_p1"])
def test_sigma_point_refusals(golden, name):
    from dust_amd import _lib as L

    g, s = golden("ut_" + name), ROLLOUT_BY_TAG[name]
    f = FAMILY[s["family"]]
    w_ctrl = (0.1,) * f["da"]

    def refused(c, **kw):
        c.set_a_mat(g["a_mat0"])
        with pytest.raises(L.DustError) as e:
            c.disco_forward(g["state"], g["ext_actions"], params=g["sigma_points"], **kw)
        assert e.value.status == L.ERR_UNSUPPORTED

    def works(c):
        c.set_a_mat(g["a_mat0"])
        assert np.isfinite(c.disco_forward(g["state"], g["ext_actions"], params=g["sigma_points"])[0]).all()

    c = _ctx(s, w_quad_ctrl=w_ctrl)  # a control weight: the reference's cost call raises (disco.py:306-309)
    c.set_param_weights(g["loc_weights"])
    refused(c)
    c.set_param_weights(None)
    works(c)
    c.close()
    c = _ctx(s, ctrl_penalty=0.5)  # a_reg != 0: the reference's control cost reads sample 0 only (disco.py:338-340)
    assert c.cfg.a_reg != 0.0
    c.set_param_weights(g["loc_weights"])
    refused(c)
    c.set_param_weights(None)
    works(c)
    c.close()
    c = _ctx(s)  # binary16 storage
    c.set_param_weights(g["loc_weights"])
    refused(c, want_states=True, store_f16=True)
    c.set_a_mat(g["a_mat0"])
    assert _err(c.disco_forward(g["state"], g["ext_actions"], params=g["sigma_points"])[0], g, "costs") < float(g["tol_costs"])
    with pytest.raises(L.DustError) as e:  # a scale without weights, a negative scale
        c.set_sigma_scale(-1.0)
    assert e.value.status == L.ERR_INVALID
    c.close()


def _filter(family, x, bw, up=None):
    from dust_amd import MpfContext

    up = up or SIGMA_UP[(family, x.shape[1])]
    if family == "pendulum":
        return MpfContext(x, np.array([3.0, 0.0], np.float32), uncertain_params=up, init_bw=bw)
    if family == "skid":
        return MpfContext(x, np.zeros(5, np.float32), model="skid_steer", uncertain_params=up, init_bw=bw, dt=0.1)
    return MpfContext(x, np.zeros(4, np.float32), model="cartpole", uncertain_params=up, init_bw=bw, dt=cpc.DT)


def test_dual_tick_refuses_weights_without_a_scale_and_a_wrong_sample_count(golden):
    from dust_amd import _lib as L

    g, s = golden("ut_cartpole_tick"), TICK_BY_TAG["cartpole_tick"]
    x = cpc.particles(s["up"], 16, False, 3, 0.1)
    m = _filter("cartpole", x, 0.05, up=s["up"])

    def ctx(**kw):
        c = _ctx(s, kernel="K1", lr=s["lr"], alpha=s["alpha"], **kw)
        c.set_theta(g["theta0"]); c.set_prior(g["mu0"]); c.set_a_mat(g["theta0"])
        return c

    c = ctx()
    c.set_param_weights(g["loc_weights"])
    with pytest.raises(L.DustError) as e:  # weights, no scale: the sigma points cannot be formed (and random draws are not them)
        c.dual_tick(m, g["state"], None, 1)
    assert e.value.status == L.ERR_UNSUPPORTED
    c.set_sigma_scale(float(g["sigma_scale"]))
    a_seq, pw, _ = c.dual_tick(m, g["state"], None, 1)
    assert np.isfinite(a_seq).all() and abs(float(pw.sum()) - 1.0) < 1e-4
    c.set_param_weights(None)  # clears the scale with the weights
    c.set_param_weights(g["loc_weights"])
    with pytest.raises(L.DustError) as e:
        c.dual_tick(m, g["state"], None, 1)
    assert e.value.status == L.ERR_UNSUPPORTED
    c.close()
    c = ctx(M=4)  # M != 2P + 1
    c.set_param_weights(np.full(4, 0.25, np.float32))
    c.set_sigma_scale(0.5)
    with pytest.raises(L.DustError) as e:
        c.dual_tick(m, g["state"], None, 1)
    assert e.value.status == L.ERR_INVALID
    c.close()
    m.close()


# ------------------------------------------------------------------------------------------------ 5. sigma points of the filter
@pytest.mark.parametrize("name", SIGMA_NAMES)
def test_filter_sigma_points_vs_reference(golden, name):
    """dust_mpf_sigma_points against compute_sigma_points(prior.mean, prior.variance.diag()) of the reference's MPF.update_prior(bw), on
    every family's filter that carries P parameters; two calls give the same bits."""
    from dust_amd import _lib as L

    g, s = golden("ut_sigma_mpf_" + name), SIGMA_BY_TAG[name]
    ran = 0
    for family in ("pendulum", "skid", "cartpole"):
        if (family, s["P"]) not in SIGMA_UP:
            continue
        m = _filter(family, g["x"], s["bw"])
        a, b = m.sigma_points(float(g["sigma_scale"])), m.sigma_points(float(g["sigma_scale"]))
        e = _err(a, g, "points")
        print("%s %s %.1e/%.1e" % (name, family, e, float(g["tol_points"])))
        assert a.shape == (2 * s["P"] + 1, s["P"]) and np.array_equal(a, b)
        assert e < float(g["tol_points"]), (name, family, e)
        assert elemerr(a, g["points_nobw"]) >= 5 * float(g["tol_points"])  # (the bandwidth is in the variance)
        with pytest.raises(L.DustError) as err:
            m.sigma_points(0.0)
        assert err.value.status == L.ERR_INVALID
        m.close()
        ran += 1
    assert ran >= 1


# ------------------------------------------------------------------------------------------------ 6. the fused dual tick
def _plant(family, st, a):
    from dust_amd.models import CartPoleModel, PendulumModel

    if family == "cartpole":
        m = CartPoleModel(dt=cpc.DT, **cpc.TRUE)
        return m.step(torch.from_numpy(np.asarray(st, np.float32)).reshape(1, 4), torch.from_numpy(np.asarray(a, np.float32)).reshape(1, 1)).reshape(-1).numpy()
    m = PendulumModel(length=0.8, mass=1.25)
    return m.step(torch.from_numpy(np.asarray(st, np.float32)).reshape(1, 2), torch.from_numpy(np.asarray(a, np.float32)).reshape(1, 1)).reshape(-1).numpy()


@pytest.mark.parametrize("family", ["pendulum", "cartpole"])
def test_dual_tick_over_sigma_points_equals_its_pieces(family):
    """dust_dual_tick over a sigma-point controller is its pieces called one by one - dust_mpf_optimize, dust_mpf_sigma_points,
    dust_svmpc_tick fed those points for each SVGD iteration - bit for bit, over three control periods; and it is NOT what random
    draws from the filter's prior give (what the call computed before it looked at the weights)."""
    from dust_amd import Context, MpfContext

    N, S, H, K, Mp = 16, 16, 8, 2, 130
    rng = np.random.default_rng(13)
    mu = (0.4 * rng.standard_normal((N, H, 1))).astype(np.float32)
    th = (mu + 0.3 * rng.standard_normal((N, H, 1))).astype(np.float32)
    if family == "cartpole":
        up, s0 = ("mass_pole", "length"), np.array(cpc.STATE0, np.float32)
        x0 = cpc.particles(up, Mp, False, 91, 0.15)
        ckw = dict(model="cartpole", sigma_a=cpc.SIGMA_A, sigma_p=cpc.SIGMA_A, alpha=0.25, goal=cpc.GOAL, w_quad_state=cpc.W_STATE,
                   w_quad_term=cpc.W_TERM, w_quad_ctrl=(0.0,))
        mkw = dict(model="cartpole", obs_std=0.05, lr=1e-4, init_bw=0.05)
    else:
        up, s0 = ("length", "mass"), np.array([3.0, 0.0], np.float32)
        x0 = (1.0 + 0.15 * rng.standard_normal((Mp, 2))).astype(np.float32)
        ckw = dict(model="pendulum", sigma_a=2.0, sigma_p=2.0, alpha=1.0)
        mkw = dict(obs_std=0.1, lr=1e-4, init_bw=0.1)
    P = len(up)
    w, scale = weights(P)

    def make():
        c = Context(N=N, S=S, M=2 * P + 1, H=H, kernel="K1", lr=0.05, uncertain_params=up, seed=5, **ckw)
        c.set_theta(th); c.set_prior(mu); c.set_a_mat(th)
        c.set_param_weights(w.astype(np.float32))
        c.set_sigma_scale(scale)
        return c, MpfContext(x0, s0, uncertain_params=up, **mkw)

    ca, ma = make()
    cb, mb = make()
    cr, mr = make()  # random draws in place of the sigma points: the weights cleared for the dual tick is not an option, so feed draws by hand
    sa, prev = s0, None
    for t in range(3):
        a1, p1, bw1 = ca.dual_tick(ma, sa, prev, K, mpf_steps=6, mpf_bw=None, seed=100 + t)
        if prev is not None:
            bw2 = mb.silverman()
            mb.optimize(prev, sa, bw2, 6)
            assert bw1 == bw2
        pts = mb.sigma_points(scale)
        a2, p2 = cb.svmpc_tick(sa, K, None, np.repeat(pts[None], K, 0))
        assert np.isfinite(a1).all() and abs(float(p1.sum()) - 1.0) < 1e-4
        assert np.array_equal(a1, a2) and np.array_equal(p1, p2), t
        assert np.array_equal(ma.get_particles(), mb.get_particles()), t
        if t == 0:
            a3, p3 = cr.svmpc_tick(sa, K, None, mr.prior_sample(K * (2 * P + 1), 100).reshape(K, 2 * P + 1, P))
            assert not np.array_equal(p1, p3)
        prev = a1[0].copy()
        sa = _plant(family, sa, a1[0])
    assert np.array_equal(ca.get_theta(), cb.get_theta())
    assert not np.array_equal(ma.get_particles(), x0)
    for o in (ca, cb, cr, ma, mb, mr):
        o.close()


def test_dual_svmpc_over_sigma_points_fused_equals_unfused_within_the_tick_tolerance(golden):
    """DualSVMPC over a sigma-point cart-pole controller: fused (the device forms the sigma points of the filter's prior) against
    unfused (the host forms them from the same particles: equal up to rounding) within the tick fixture's tolerances; a transform with
    a custom sqrt_method stays on the unfused path."""
    from dust_amd.controllers import DualSVMPC
    from dust_amd.inference import MPF, SVMPC, ExponentiatedUtility, GaussianLikelihood, get_gmm
    from dust_amd.kernels import RBFKernel

    g, s = golden("ut_cartpole_tick"), dict(TICK_BY_TAG["cartpole_tick"], N=16, S=16, H=6)
    f = FAMILY["cartpole"]
    N, S, H, Mp = s["N"], s["S"], s["H"], 130
    rng = np.random.default_rng(21)
    mu0 = torch.tensor((0.4 * rng.standard_normal((N, H, 1))).astype(np.float32))
    init_policies = mu0 + torch.tensor((0.3 * rng.standard_normal((N, H, 1))).astype(np.float32))
    x0 = torch.tensor(cpc.particles(s["up"], Mp, False, 78, 0.15))
    init_state = torch.tensor(f["state0"])
    cov = f["sigma_a"] ** 2 * torch.eye(1)
    eps = rng.standard_normal((4, 1, S, N, H, 1)).astype(np.float32)

    def make(fused, **tf_kw):
        model = _mirror_model(s)
        ctrl = _mirror_controller(s, model, 0.5, **tf_kw)
        ctrl.a_mat = init_policies.clone()
        ctrl.return_rollouts = False
        mpf = MPF(init_particles=x0.clone(), likelihood=GaussianLikelihood(initial_obs=init_state, obs_std=0.05, model=model, log_space=False),
                  optimizer_class=torch.optim.SGD, lr=1e-4, bw=0.05, bw_scale=1.0)
        sv = SVMPC(likelihood=ExponentiatedUtility(alpha=0.25, n_samples=S, controller=ctrl, model=model), init_particles=init_policies.clone(),
                   prior=get_gmm(mu0, torch.ones(N), cov), kernel=RBFKernel(), n_particles=N, bw_scale=1.0, n_steps=1,
                   optimizer_class=torch.optim.SGD, lr=0.05)
        return DualSVMPC(sv, mpf, mpf_bw=0.05, mpf_steps=6, warm_up=0, fused=fused, seed=0)

    def plant(state, action):
        return torch.from_numpy(_plant("cartpole", state.reshape(-1).numpy(), action.reshape(-1).numpy())).reshape(1, -1)

    floor = float(np.sqrt(np.mean(g["theta_after"].astype(np.float64) ** 2)))  # (one action has no rms of its own: the fixture's particles')
    fu, un = make(True), make(False)
    custom = make(True, sqrt_method=lambda A: torch.linalg.cholesky(A).transpose(-2, -1))
    assert fu._can_fuse() and not un._can_fuse() and not custom._can_fuse()
    sf = su = init_state.reshape(1, -1)
    for t in range(3):  # the same seed on both controllers: the same device-drawn policy noise
        af, sf, pf = fu.tick(sf, plant)
        au, su, pu = un.tick(su, plant)
        assert torch.isfinite(af).all() and abs(float(pf.sum()) - 1.0) < 1e-4, t
        ea, ep = elemerr(af.numpy(), au.numpy(), floor=floor), elemerr(pf.numpy(), pu.numpy())
        print("period %d: action %.1e/%.1e  p_weights %.1e/%.1e" % (t, ea, float(g["tol_theta_after"]), ep, float(g["tol_p_weights"])))
        assert ea < float(g["tol_theta_after"]) and ep < float(g["tol_p_weights"]), t
    ac, _, pc = custom.tick(init_state.reshape(1, -1), plant)  # the unfused path, through _sigma_params on the host
    assert torch.isfinite(ac).all() and abs(float(pc.sum()) - 1.0) < 1e-4
    # the device's points are the host's up to rounding
    pts_dev = fu.mpf._dev.sigma_points(fu.controller._tf.scale)
    pts_host = fu.controller._sigma_params(fu.mpf.prior)[0][0]
    assert elemerr(pts_dev, pts_host) < TOL


# ------------------------------------------------------------------------------------------------ 7. sharding
def test_sigma_point_cartpole_sharded_equals_unsharded(golden):
    """Two shards of a sigma-point cart-pole controller against the unsharded one (the criterion of test_cartpole_sharded_equals_unsharded)"""
    from dust_amd.parallel import DeviceShard, LocalComm, tick

    g = golden("ut_cartpole_p2")
    s = dict(ROLLOUT_BY_TAG["cartpole_p2"], N=64, S=32, H=10)
    N, S, H, K, T, M = 64, 32, 10, 2, 2, 5
    rng = np.random.default_rng(5)
    mu = (0.4 * rng.standard_normal((N, H, 1))).astype(np.float32)
    th = (mu + 0.3 * rng.standard_normal((N, H, 1))).astype(np.float32)
    eps = rng.standard_normal((T, K, S, N, H, 1)).astype(np.float32)
    params = np.repeat(g["sigma_points"][None], K, 0)
    kw = context_kwargs(s, kernel="K1", lr=0.05, seed=11)
    ref = _ctx(s, kernel="K1", lr=0.05, seed=11)
    ref.set_param_weights(g["loc_weights"])
    ref.set_theta(th); ref.set_prior(mu); ref.set_a_mat(th)
    outs = [ref.svmpc_tick(g["state"], K, eps[t], params) for t in range(T)]
    rt = ref.get_theta()
    assert not np.array_equal(rt, th)
    shards = tuple(DeviceShard(dict(kw), r, 2) for r in range(2))
    for sh in shards:
        sh.ctx.set_param_weights(g["loc_weights"])
        sh.set_state(th, mu, th)
    for t in range(T):
        a_seq, pw = tick(shards, LocalComm(), g["state"], K, eps[t], params, want_outputs=True, final_gather=True)
        assert np.array_equal(a_seq, outs[t][0]), t
        assert relerr(pw, outs[t][1]) < 1e-5
    for sh in shards:
        sh.sync()
        assert elemerr(sh.ctx.get_theta(), rt) < 2e-6, sh.rank
        sh.ctx.close()
    ref.close()
