"""The skid-steer controller family on the device (csrc/skid.hpp + the regular rollout kernel's second pass) beyond the three round-3
fixtures: the reference's own MultiDISCO.forward on SkidSteerRobot at a partial second block, every column order, three log-space
columns, the scalar-event quirk, asymmetric bounds, a full 2 x 2 a_cov and ctrl_penalty != 1 (tests/golden/skid_ctrl_<tag>.npz, made by
tests/golden/make_golden_skid.py from the scenarios of tests/skid_cases.py), through the C ABI and the mirror class; device-drawn noise
under the full a_cov; whole ticks and sharded ticks with the control-regularisation term (skid-steer and cart-pole); and the range of
the shared sine / cosine (common.hpp fast_sinf / fast_cosf, rollout.hpp's branch-free Pendulum path) up to headings of 3e6.

Every fixture tolerance is the fixture's own, measured from the reference alone; a comparison takes the smaller distance to the
reference's fp32 and float64 values.
"""
import numpy as np
import pytest

import cartpole_cases
import skid_cases as cases
from helpers import RecordedDraws, elemerr, relerr

pytestmark = pytest.mark.gpu
TOL = 1e-5  # the project's stage tolerance (where no fixture carries one)


def _err(got, g, q, c):
    """elemerr against the reference's fp32 or float64 value of call c of quantity q, whichever is nearer"""
    return min(elemerr(got, g[q][c]), elemerr(got, cases.twin(g, q)[c]))


def _ctx(s, **kw):
    from dust_amd import Context

    return Context(**cases.controller_kwargs(s, **kw))


def _oracle_kw(s):
    lo, hi = s["bounds"]
    return dict(uncertain_params=s["up"], dt=s["dt"], lo=(lo, lo), hi=(hi, hi), goal=cases.GOAL, w_state=cases.W_STATE, w_term=cases.W_TERM,
                w_ctrl=cases.W_CTRL, log_space=s["log"], interleave=s["dist"] == "scalar", **s["fixed"])


def _areg_term(actions, a_seq, a_mat, a_pre, a_reg):
    """a_reg * diag(tensordot(-(actions - a_seq), a_mat @ a_pre)) (disco.py:338-346) in float64; a_pre: a [2] diagonal or a [2, 2] matrix"""
    f = lambda a: np.asarray(a, np.float64)
    pre = f(a_pre) if np.ndim(a_pre) == 2 else np.diag(f(a_pre))
    return a_reg * np.einsum("snhd,nhd->sn", -(f(actions) - f(a_seq)), f(a_mat) @ pre)


# ------------------------------------------------------------------------------------------------ 1. the fixtures through the Context
@pytest.mark.parametrize("mode", ["actions", "eps"])
@pytest.mark.parametrize("name", cases.ROLLOUT_NAMES)
def test_rollout_fixtures_vs_reference(golden, name, mode):
    """skid_rollout_kernel + the regular kernel's second pass against the reference's MultiDISCO.forward, call after call: costs, every
    rollout's states, omega, the a_mat update, a_mix from recorded actions; costs, the a_mat update and a_mix from recorded eps, where the
    device forms actions = theta + L eps itself - in skid.hpp for the costs, in the regular kernel's tile for everything downstream -
    bit for bit.  With the fixture's one thing ignored the reference is >= 10 tolerances away, the device >= 5."""
    g, s = golden("skid_ctrl_" + name), cases.ROLLOUT_BY_TAG[name]
    lead = cases.lead_quantity(s)
    c = _ctx(s)
    c.set_a_mat(g["a_mat0"])
    c.set_a_seq(g["a_seq0"])
    if mode == "eps":
        c.set_theta(g["a_mat0"])
    errs, power = {}, []
    for k in range(s["calls"]):
        params = g["params"][k] if s["up"] else None
        if mode == "actions":
            costs, states, _, omega = c.disco_forward(g["state"], g["ext_actions"][k], params=params, want_states=True)
            got = dict(costs=costs, states=states, omega=omega, a_mat1=c.get_a_mat(), a_mix=c.get_a_mix())
        else:
            costs, actions = c.likelihood_sample(g["state"], g["eps"][k], params, want_actions=True)
            assert np.array_equal(actions, g["ext_actions"][k]), "theta + L eps must be bit-exact"
            assert np.array_equal(c.get_costs(), costs)
            got = dict(costs=costs, a_mat1=c.get_a_mat(), a_mix=c.get_a_mix())
        for q, v in got.items():
            errs[q] = max(errs.get(q, 0.0), _err(v, g, q, k))
        if lead in got:
            power.append(elemerr(g[lead + "_off"][k], got[lead]))
    c.close()
    print("%s [%s] " % (name, mode) + "  ".join("%s %.1e/%.1e" % (q, e, float(g["tol_" + q])) for q, e in errs.items()))
    for q, e in errs.items():
        assert e < float(g["tol_" + q]), (name, mode, q, e, float(g["tol_" + q]))
    assert max(elemerr(a, b) for a, b in zip(g[lead + "_off"], g[lead])) >= 10 * float(g["tol_" + lead])
    if power:
        assert max(power) >= 5 * float(g["tol_" + lead]), (name, mode, power)


@pytest.mark.parametrize("name", ["areg", "fullcov", "scalar"])
def test_rollout_fixtures_through_the_mirror_class(golden, name):
    """The same fixtures through `MultiDISCO(..., ctrl_penalty=, a_cov=).forward(state, SkidSteerRobot(...), params_dist, ext_actions=)`
    with the recorded dynamics samples replayed: the class hands ctrl_penalty, a_seq, the full a_cov, the bounds and the scalar-event
    flag of the distribution to the device."""
    import torch
    import torch.distributions as dist

    from dust_amd.controllers import MultiDISCO
    from dust_amd.costs import QuadraticCost
    from dust_amd.models import SkidSteerRobot

    g, s = golden("skid_ctrl_" + name), cases.ROLLOUT_BY_TAG[name]
    model = SkidSteerRobot(delta_t=s["dt"], uncertain_params=s["up"], min_wheel_speed=s["bounds"][0], max_wheel_speed=s["bounds"][1], **s["fixed"])
    cost = QuadraticCost(cases.GOAL, cases.W_STATE, cases.W_TERM, cases.W_CTRL)
    ctrl = MultiDISCO(model.observation_space, model.action_space, s["H"], s["N"], s["S"], temperature=cases.TEMPERATURE, ctrl_penalty=s["ctrl_penalty"],
                      a_cov=torch.tensor(cases.a_cov_of(s), dtype=torch.float), inst_cost_fn=cost.inst_cost, term_cost_fn=cost.term_cost,
                      params_sampling=True, params_samples=s["M"], params_log_space=s["log"])
    ctrl.a_mat = torch.tensor(g["a_mat0"])
    ctrl.a_seq = torch.tensor(g["a_seq0"])
    if s["dist"] == "scalar":
        pdist = dist.Normal(s["loc"][0], s["scale"][0])
        draws = [p.reshape(-1) for p in g["params"]]
    else:
        pdist = dist.Independent(dist.Uniform(torch.tensor(s["lo"]), torch.tensor(s["hi"])), 1)
        draws = list(g["params"])
    ctrl.draw_source = RecordedDraws(params=draws)
    costs, states, actions, omega, _ = ctrl.forward(torch.tensor(g["state"]), model, pdist, ext_actions=torch.tensor(g["ext_actions"][0]))
    got = dict(costs=costs.numpy(), states=states.numpy(), omega=omega.numpy(), a_mat1=ctrl.a_mat.numpy(), a_mix=ctrl.a_mix.numpy())
    errs = {q: _err(got[q], g, q, 0) for q in cases.ROLLOUT_QUANT}
    print("%s [mirror] " % name + "  ".join("%s %.1e/%.1e" % (q, e, float(g["tol_" + q])) for q, e in errs.items()))
    for q, e in errs.items():
        assert e < float(g["tol_" + q]), (name, q, e, float(g["tol_" + q]))
    lead = cases.lead_quantity(s)
    assert elemerr(g[lead + "_off"][0], got[lead]) >= 5 * float(g["tol_" + lead])


# ------------------------------------------------------------------------------------------------ 2. device-drawn noise, full a_cov
def test_device_noise_with_a_full_a_cov():
    """Policy noise drawn on the device under a full 2 x 2 a_cov, at the shape of `ragged` (a partial second block; D = 30: the last
    Philox block of a row is partial).  skid.hpp draws the actions for the costs, the regular kernel draws them again for the weights,
    the score and the a_mat update: the fetched actions (the second kernel's) replayed through the oracle give the first kernel's costs,
    and omega, the a_mat update and the likelihood score recomputed in float64 from the fetched actions and the returned costs are the
    device's - so both kernels drew the same actions.  Whitened with L they are standard normal; another seed draws others."""
    from oracle import Oracle

    s = dict(cases.ROLLOUT_BY_TAG["ragged"], a_cov=cases.FULL_COV)
    N, S, H, M = s["N"], s["S"], s["H"], s["M"]
    rng = np.random.default_rng(17)
    th = (0.25 * rng.standard_normal((N, H, 2))).astype(np.float32)
    params = rng.uniform(s["lo"], s["hi"], (M, 2)).astype(np.float32)
    state = np.array(cases.STATE0, np.float32)
    f = lambda a: np.asarray(a, np.float64)
    drawn = []
    for seed in (9, 10):
        c = _ctx(s, seed=seed)
        c.set_theta(th); c.set_a_mat(th)
        costs, _, actions, omega = c.disco_forward(state, None, params=params, want_actions=True)  # (around a_mat: eps = actions - a_mat)
        gl, _ = c.get_score_parts()
        a_mat1, a_mix = c.get_a_mat(), c.get_a_mix()
        sig2 = np.array([float(c.cfg.sigma_a[d]) ** 2 for d in range(2)])
        c.close()
        drawn.append(actions)
        e = elemerr(costs, Oracle.skid_rollout_cost(state, actions, params=params, **_oracle_kw(s)))
        lc = -(f(costs) - f(costs).min()) / cases.TEMPERATURE
        eta = lc.max(0) + np.log(np.exp(lc - lc.max(0)).sum(0))
        om = np.exp(lc - eta)
        eps = f(actions) - f(th)
        delta = np.einsum("sn,snhd->nhd", om, eps)
        errs = dict(costs=e, omega=relerr(omega, om), a_mat1=relerr(a_mat1, f(th) + delta), score=elemerr(gl, delta / sig2),
                    a_mix=relerr(a_mix, np.exp(eta - (eta.max() + np.log(np.exp(eta - eta.max()).sum())))))
        print("device noise, full a_cov, seed %d: " % seed + "  ".join("%s %.1e" % kv for kv in errs.items()))
        # (the bounds of test_gpu_parity.py for the same quantities: costs TOL, omega 2e-4, a_mat 1e-4, score TOL, a_mix 2e-4)
        assert errs["costs"] < TOL and errs["omega"] < 2e-4 and errs["a_mat1"] < 1e-4 and errs["score"] < TOL and errs["a_mix"] < 2e-4, errs
        L = np.linalg.cholesky(f(np.asarray(cases.FULL_COV, np.float32)))
        z = np.linalg.solve(L, eps.reshape(-1, 2).T)  # [2, n]: (actions - theta) L^-T, column by column
        n = z.shape[1]
        assert np.all(np.abs(z.mean(1)) < 5 / np.sqrt(n)), z.mean(1)
        cov = np.cov(z)
        assert abs(cov[0, 0] - 1) < 5 * np.sqrt(2.0 / n) and abs(cov[1, 1] - 1) < 5 * np.sqrt(2.0 / n) and abs(cov[0, 1]) < 5 / np.sqrt(n), cov
    assert not np.array_equal(drawn[0], drawn[1])


# ------------------------------------------------------------------------------------------------ 3. whole ticks with a_reg != 0
@pytest.mark.parametrize("kernel,opt", [("K1", "SGD"), ("K2", "Adam")])
def test_skid_ticks_with_ctrl_penalty_vs_oracle(kernel, opt):
    """Two SVGD iterations and forward() with ctrl_penalty = 0.6 at the shape of test_skid_steer_svmpc_ticks_vs_oracle, against the
    oracle's composition (skid rollouts -> score -> phi -> optimiser -> forward) with the control-regularisation term added to the
    oracle's state costs in float64 here - through the a_mat every sample leaves behind (disco.py:387-392)."""
    from oracle import Oracle

    s = cases.ROLLOUT_BY_TAG["areg"]
    N, S, H, M, K = 12, 32, 10, 3, 2
    rng = np.random.default_rng(3)
    sig, alpha = 0.3, 0.5
    lr = 0.05 if opt == "SGD" else 0.01
    temp = 1.0 / alpha
    a_reg = temp * (1 - cases.CTRL_PENALTY)
    mu = (0.2 * rng.standard_normal((N, H, 2))).astype(np.float32)
    theta = (mu + 0.1 * rng.standard_normal((N, H, 2))).astype(np.float32)
    state = np.array(cases.STATE0, np.float32)
    c = _ctx(dict(s, N=N, S=S, H=H, M=M), kernel=kernel, optimizer=opt, lr=lr, alpha=alpha, temperature=temp, seed=9)
    c.set_theta(theta); c.set_prior(mu); c.set_a_mat(theta)
    eps = rng.standard_normal((K, S, N, H, 2)).astype(np.float32)
    params = np.stack([rng.uniform(s["lo"], s["hi"], (M, 2)) for _ in range(K)]).astype(np.float32)
    a_seq, pw = c.svmpc_tick(state, K, eps=eps, params=params)
    assert c.tick_stats()["tick2"] == 0
    o = Oracle(model="particle", N=N, S=S, M=1, H=H)  # (score / phi / forward do not touch the model)
    sg = np.full(2, sig, np.float32)
    a_pre = 1.0 / (sg.astype(np.float64) ** 2)
    kw = _oracle_kw(s)
    th, mix, a_mat, zero = theta.copy(), np.ones(N, np.float32), theta.copy(), np.zeros((H, 2), np.float32)
    m, v = np.zeros_like(th), np.zeros_like(th)
    for k in range(K):
        actions = o.sample_actions(th, eps[k], sg)
        plain = Oracle.skid_rollout_cost(state, actions, params=params[k], **kw)
        term = _areg_term(actions, zero, a_mat, a_pre, a_reg)
        costs = (plain.astype(np.float64) + term).astype(np.float32)
        if k == K - 1:
            e = elemerr(c.get_costs(), costs)
            print("tick %s %s: costs %.1e, the term's share %.2f" % (kernel, opt, e, elemerr(plain, costs)))
            assert e < TOL and elemerr(plain, costs) > 100 * TOL
        _, a_mat, _ = o.disco_weights(costs, actions, zero, temp, a_mat)
        _, _, sc = o.score(th, mu, mix, sg, costs, actions, alpha, sg)
        if opt == "SGD":
            th = o.sgd(th, o.phi_k1(th, sc) if kernel == "K1" else o.phi_k2(th, sc)[0], lr)
        else:
            th, m, v = o.adam(th, o.phi_k1(th, sc) if kernel == "K1" else o.phi_k2(th, sc)[0], m, v, k + 1, lr)
    r = o.forward(costs, th, mu, mix, sg, alpha)
    assert elemerr(c.get_theta(), r["theta"]) < 1e-4
    assert np.abs(pw - r["p_weights"]).max() < 2e-3
    # device Philox noise: the draws fetched as actions, replayed through the oracle, the term from the context's own a_mat / a_seq
    a_mat, a_seq_now = c.get_a_mat(), c.get_a_seq()
    costs_dev, actions = c.likelihood_sample(state, None, params[0], want_actions=True)
    plain = Oracle.skid_rollout_cost(state, actions, params=params[0], **kw)
    ref = (plain.astype(np.float64) + _areg_term(actions, a_seq_now, a_mat, a_pre, a_reg)).astype(np.float32)
    assert elemerr(costs_dev, ref) < TOL and elemerr(plain, ref) > 100 * TOL
    c.close()


def test_particle_first_pass_adds_its_control_term_once():
    """The third first pass, particle_general.hpp (stored states under control noise), adds the control-regularisation term itself: the
    second pass must leave its costs alone.  Costs against the oracle with ctrl_penalty = 0.5 in an obstacle-free scene (costs of
    order 10: the term, and a second copy of it, are far over the tolerance)."""
    from oracle import Oracle
    from test_gpu_ctrl_noise import _context, _ctrl_z, _scene

    S, N, M, H = 64, 3, 4, 23
    ctx, ora, theta, params, state, grid = _scene(S, N, M, H, "free", (0.6, 0.4), ctrl_penalty=0.5)
    c = _context(ctx, grid, theta)
    rng = np.random.default_rng(11)
    actions = (theta[None] + rng.standard_normal((S, N, H, 2))).astype(np.float32)
    costs, states, _, _ = c.disco_forward(state, actions, params, want_states=True)
    assert np.array_equal(c.get_costs(), costs)
    a_reg = float(np.float32(float(c.cfg.temperature) * 0.5))
    c.close()
    z = _ctrl_z("general", S, N, M, H)
    o = Oracle(**ora)
    ref, ref_states = o.rollout_cost(state, actions, params, a_reg, theta, None, np.ones(2, np.float32), want_states=True, ctrl_noise=z)
    plain = o.rollout_cost(state, actions, params, ctrl_noise=z)
    e = elemerr(costs, ref)
    print("particle_general with ctrl_penalty 0.5: costs %.1e, the term's share %.2f" % (e, elemerr(plain, ref)))
    assert elemerr(plain, ref) > 100 * TOL
    assert e < TOL, e
    assert np.abs(states - ref_states).max() < 1e-5 * max(1.0, np.abs(ref_states).max())


# ------------------------------------------------------------------------------------------------ 4. sharding with a_reg != 0
@pytest.mark.parametrize("family", ["skid_steer", "cartpole"])
def test_sharded_equals_unsharded_with_ctrl_penalty(family):
    """World 2 equals unsharded with ctrl_penalty = 0.6 (the criterion and bounds of test_skid_steer_sharded_equals_unsharded /
    test_cartpole_sharded_equals_unsharded): row n of a_mat in the term is the GLOBAL particle index."""
    from dust_amd import Context
    from dust_amd.parallel import DeviceShard, LocalComm, tick

    N, S, H, M, K, T = 64, 32, 10, 3, 2, 2
    rng = np.random.default_rng(5)
    if family == "skid_steer":
        s = dict(cases.ROLLOUT_BY_TAG["areg"], N=N, S=S, H=H, M=M)
        kw = cases.controller_kwargs(s, kernel="K1", lr=0.05, alpha=0.5, temperature=2.0, seed=11)
        da, scale, state = 2, (0.2, 0.1), np.array(cases.STATE0, np.float32)
    else:
        s = dict(cartpole_cases.ROLLOUT_BY_TAG["ragged"], N=N, S=S, H=H, M=M, ctrl_penalty=0.6)
        kw = cartpole_cases.controller_kwargs(s, kernel="K1", lr=0.05, seed=11)
        da, scale, state = 1, (0.4, 0.3), np.array(cartpole_cases.STATE0, np.float32)
    mu = (scale[0] * rng.standard_normal((N, H, da))).astype(np.float32)
    th = (mu + scale[1] * rng.standard_normal((N, H, da))).astype(np.float32)
    eps = rng.standard_normal((T, K, S, N, H, da)).astype(np.float32)
    params = np.stack([[rng.uniform(s["lo"], s["hi"], (M, 2)) for _ in range(K)] for _ in range(T)]).astype(np.float32)
    ref = Context(**kw)
    assert float(ref.cfg.a_reg) != 0.0
    ref.set_theta(th); ref.set_prior(mu); ref.set_a_mat(th)
    outs = [ref.svmpc_tick(state, K, eps[t], params[t]) for t in range(T)]
    rt = ref.get_theta()
    assert not np.array_equal(rt, th)
    world = 2
    shards = tuple(DeviceShard(dict(kw), r, world) for r in range(world))
    for sh in shards:
        sh.set_state(th, mu, th)
    for t in range(T):
        a_seq, pw = tick(shards, LocalComm(), state, K, eps[t], params[t], want_outputs=True, final_gather=True)
        assert np.array_equal(a_seq, outs[t][0]), t
        assert relerr(pw, outs[t][1]) < 1e-5
    for sh in shards:
        sh.sync()
        assert elemerr(sh.ctx.get_theta(), rt) < 2e-6, sh.rank
        sh.ctx.close()
    ref.close()


# ------------------------------------------------------------------------------------------------ 5. the range of sine and cosine
HEADINGS = [0.5, -2.5, 100.0, -1e3, 3e4, -99999.0, 1e5, 3e6]


@pytest.mark.parametrize("heading", HEADINGS)
def test_skid_step_over_the_heading_range(heading):
    """One SkidSteerRobot.step from a start heading of up to 3e6 rad (fast_sinf / fast_cosf: Cody-Waite reduction below 1e5, libm from
    there on): x' and y' of the stored states against float64 numpy on the same fp32 inputs.  The bound is derived: per entry
    8 * 2^-24 * (|x| + |fwd| + |lat|) - three fp32 roundings ((x + fwd cos) - lat sin: two products, two sums, the first sum's error
    carried) and 1.5 ulp of each trig value, with a factor of two over their sum.  A wrong quadrant misses it by five orders."""
    N, S, H = 2, 64, 1
    s = dict(cases.ROLLOUT_BY_TAG["bounds"], N=N, S=S, H=H, M=1, bounds=cases.BOUNDS, dt=cases.DT, fixed=dict(cases.DEFAULTS))
    rng = np.random.default_rng(int(abs(heading)) % 1000 + 1)
    actions = rng.uniform(-0.6, 0.6, (S, N, H, 2)).astype(np.float32)
    state = np.array([0.3, -0.2, heading, 0.0, 0.0], np.float32)
    c = _ctx(s)
    c.set_a_mat(np.zeros((N, H, 2), np.float32))
    _, states, _, _ = c.disco_forward(state, actions, want_states=True)
    c.close()
    assert np.array_equal(states[0, :, :, 0], np.broadcast_to(state, (S, N, 5)))
    nxt = states[0, :, :, 1].astype(np.float64)  # [S, N, 5]
    f32 = np.float32
    th = float(state[2])
    a = np.clip(actions[:, :, 0].astype(np.float64), -0.5, 0.5)
    wr, ad, xi, dt = (float(f32(v)) for v in (0.0625, 0.475, 0.2, cases.DT))
    lin = (a[..., 0] + a[..., 1]) * float(f32(np.pi)) * wr
    ang = (a[..., 0] - a[..., 1]) * 2 * float(f32(np.pi)) * wr / ad
    ulp = 2.0 ** -24
    assert np.all(np.abs(nxt[..., 3] - lin) <= 4 * ulp * np.abs(lin)) and np.all(np.abs(nxt[..., 4] - ang) <= 5 * ulp * np.abs(ang))  # (3 / 4 roundings)
    # forward and lateral shifts from the STORED speeds, in the kernel's fp32 order (skid.hpp): what is under test is the rotation
    lin32, ang32 = states[0, :, :, 1, 3], states[0, :, :, 1, 4]
    fwd = (lin32 * f32(dt)).astype(np.float64)
    lat = (((-ang32) * f32(xi)) * f32(dt)).astype(np.float64)
    x_ref = float(state[0]) + fwd * np.cos(th) - lat * np.sin(th)
    y_ref = float(state[1]) + fwd * np.sin(th) + lat * np.cos(th)
    bx = 8 * ulp * (abs(float(state[0])) + np.abs(fwd) + np.abs(lat))
    by = 8 * ulp * (abs(float(state[1])) + np.abs(fwd) + np.abs(lat))
    ex, ey = np.abs(nxt[..., 0] - x_ref), np.abs(nxt[..., 1] - y_ref)
    print("heading %g: x' %.2f of its bound, y' %.2f (shifts up to %.3f)" % (heading, (ex / bx).max(), (ey / by).max(), np.abs(fwd).max()))
    assert np.abs(fwd).max() > 5e4 * bx.max()  # (a wrong quadrant moves an entry by about its shift: some five orders over the bound)
    assert np.all(ex <= bx) and np.all(ey <= by), ((ex / bx).max(), (ey / by).max())
    th1 = (f32(state[2]) + ang32 * f32(dt)).astype(np.float32)
    assert np.array_equal(states[0, :, :, 1, 2], th1)


# (angles of a few radians are every other test's; there theta_1 has the resolution of the velocity and the stability condition below says nothing)
# start angles on both sides of the branch-free path's 5e4 switch (|theta0| + max_speed dt H = |theta0| + 0.4 < 5e4) and of fast_sinf's 1e5
PEND_ANGLES = [2.0e4, -3.0e4, 4.9e4, -4.9e4, 49999.5, -49999.5, 49999.75, -5.0e4, 5.0e4, 9.9e4, -99999.0, 1.0e5, -1.0e5, 1.3e5, -3.0e6]


def pendulum_theta1_is_stable(o, state, actions, params):
    """On the host: the oracle's theta_1 of every rollout is unchanged when the first step's velocity is moved by up to +-4 ulp - at 1e5
    rad one fp32 step of theta is 2^-7 rad, and a rounding tie in theta_0 + thd dt would decide the terminal cost."""
    _, st = o.rollout_cost(state, actions, params, want_states=True)
    th0, th1, thd = np.float32(state[0]), st[..., 1, 0], st[..., 1, 1]
    dt = np.float32(0.05)
    assert np.array_equal((th0 + thd * dt).astype(np.float32), th1), "the host model of theta_1 is not the oracle's"
    for direction in (-np.inf, np.inf):
        v = thd.copy()
        for _ in range(4):
            v = np.nextafter(v, np.float32(direction))
            if not np.array_equal((th0 + v * dt).astype(np.float32), th1):
                return False
    return True


def pendulum_case(angle):
    N, S, H, M = 4, 64, 1, 3
    rng = np.random.default_rng(int(abs(angle)) % 977 + 3)
    theta = (1.5 * rng.standard_normal((N, H, 1))).astype(np.float32)
    eps = rng.standard_normal((S, N, H, 1)).astype(np.float32)
    params = rng.uniform(0.7, 1.3, (M, 2)).astype(np.float32)
    state = np.array([angle, 1.5], np.float32)
    return N, S, H, M, theta, eps, params, state


def test_pendulum_costs_over_the_angle_range():
    """One Pendulum step and its costs (H = 1, costs only: the branch-free trig path is eligible below the switch) from start angles on
    both sides of the 5e4 switch and of 1e5, in both signs, with M = 3 dynamics samples (the packed two-sample loop and the one-sample
    loop), against the oracle at TOL.  Only angles whose theta_1 no rounding tie decides are compared (pendulum_theta1_is_stable); at most
    two may drop out - on the machine the list was chosen on none does."""
    from dust_amd import Context
    from oracle import Oracle

    used = 0
    for angle in PEND_ANGLES:
        N, S, H, M, theta, eps, params, state = pendulum_case(angle)
        o = Oracle(model="pendulum", N=N, S=S, M=M, H=H, uncertain_params=("length", "mass"))
        sg = np.full(1, 2.0, np.float32)
        actions = o.sample_actions(theta, eps, sg)
        if not pendulum_theta1_is_stable(o, state, actions, params):
            continue
        used += 1
        c = Context(model="pendulum", N=N, S=S, M=M, H=H, uncertain_params=("length", "mass"), sigma_a=2.0, sigma_p=2.0)
        c.set_theta(theta); c.set_a_mat(theta)
        costs = c.likelihood_sample(state, eps, params)
        c.close()
        ref = o.rollout_cost(state, actions, params)
        e = elemerr(costs, ref)
        print("pendulum theta0 %g: costs %.1e" % (angle, e))
        assert e < TOL, (angle, e)
    assert used >= len(PEND_ANGLES) - 2, used
