"""The cart-pole family on the device (csrc/cartpole.hpp, mpf.hpp mpf_cart_score), through the C ABI and the mirror classes, against
the reference's own MultiDISCO / SVMPC / MPF on its CartPoleModel (tests/golden/cartpole_*.npz and mpf_cartpole_*.npz, made by
tests/golden/make_golden_cartpole.py and make_golden_mpf_cartpole.py; the scenarios are data in tests/cartpole_cases.py).  The oracle has
no cart-pole: the reference fixtures are the independent side, and where the reference is absent (device-drawn noise) the host
`CartPoleModel.step`, which tests/test_cartpole_cpu.py pins bit-equal to the reference's.

Every tolerance is the fixture's own, measured from the reference alone (one-ulp moves of the inputs, float64 runs); a comparison takes
the smaller distance to the reference's fp32 and float64 values.  As in test_gpu_mpf_sizes.py the three forms of the filter's
optimisation kernel (single / poll / counter) are selected by the development switches and asserted through stats().
"""
import copy
import ctypes as C

import numpy as np
import pytest
import torch

from cartpole_cases import (BY_TAG, DT, GOAL, NAMES, P3, ROLLOUT_BY_TAG, ROLLOUT_NAMES, ROLLOUT_QUANT, SIGMA_A, SWEEP_SIZES, TICK_BY_TAG, TICK_NAMES,
                            TRUE, W_CTRL, W_STATE, W_TERM, controller_kwargs, lead_quantity, model_kwargs, particles, sweep_scenario, twin)
from helpers import elemerr, mpf_size_disp_err, mpf_size_err, relerr
from test_gpu_mpf_sizes import FORMS, _served, _set_form

pytestmark = pytest.mark.gpu
TOL = 1e-5  # the project's stage tolerance (where no fixture carries one)


def _err(got, g, q):
    """elemerr against the reference's fp32 or float64 value of quantity q, whichever is nearer"""
    return min(elemerr(got, g[q]), elemerr(got, twin(g, q)))


def _ctx(s, **kw):
    from dust_amd import Context

    return Context(**controller_kwargs(s, **kw))


# ------------------------------------------------------------------------------------------------ 1. the rollout family
@pytest.mark.parametrize("mode", ["actions", "eps"])
@pytest.mark.parametrize("name", ROLLOUT_NAMES)
def test_rollout_family_vs_reference(golden, name, mode):
    """cartpole_rollout_kernel + the regular kernel's weights stage against the reference's MultiDISCO.forward: costs, every rollout's
    states, omega, the a_mat update, a_mix - from recorded actions, and the costs from recorded eps (actions = theta + L eps, bit for bit)."""
    g, s = golden("cartpole_" + name), ROLLOUT_BY_TAG[name]
    c = _ctx(s)
    c.set_a_seq(g["a_seq0"])
    params = g["params"] if s["up"] else None
    if mode == "actions":
        c.set_a_mat(g["a_mat0"])
        costs, states, _, omega = c.disco_forward(g["state"], g["ext_actions"], params=params, want_states=True)
        got = dict(costs=costs, states=states, omega=omega, a_mat1=c.get_a_mat(), a_mix=c.get_a_mix())
        errs = {q: _err(got[q], g, q) for q in ROLLOUT_QUANT}
        lead = lead_quantity(s)  # the fixture's power: with its one thing ignored the reference and the device are both >= 10 tolerances away
        assert elemerr(g[lead + "_off"], g[lead]) >= 10 * float(g["tol_" + lead])
        assert elemerr(g[lead + "_off"], got[lead]) >= 9 * float(g["tol_" + lead])
    else:
        c.set_theta(g["a_mat0"])
        c.set_a_mat(g["a_mat0"])
        costs, actions = c.likelihood_sample(g["state"], g["eps"], params, want_actions=True)
        assert np.array_equal(actions, g["ext_actions"]), "theta + L eps must be bit-exact"
        errs = dict(costs=_err(costs, g, "costs"))
        assert np.array_equal(c.get_costs(), costs)
    c.close()
    print("%s [%s] " % (name, mode) + "  ".join("%s %.1e/%.1e" % (q, e, float(g["tol_" + q])) for q, e in errs.items()))
    for q, e in errs.items():
        assert e < float(g["tol_" + q]), (name, mode, q, e, float(g["tol_" + q]))


# ------------------------------------------------------------------------------------------------ 2. whole ticks
@pytest.mark.parametrize("name", TICK_NAMES)
def test_ticks_vs_reference(golden, name):
    """Two SVGD iterations and forward() against the reference's SVMPC (K1 + SGD, K2 iid_mp, K1 + Adam), stage by stage: score and phi
    with the reference's costs and actions injected downstream of the softmax (dust_svmpc_phi, as test_phi_update_vs_reference), the
    updated particles and costs from the recorded draws, then forward() from the reference's particles (as test_forward_vs_reference):
    log_l, log_p, p_weights, the same argmax, a_seq bit for bit."""
    g, s = golden("cartpole_" + name), TICK_BY_TAG[name]
    K, N = int(g["K"]), s["N"]
    mix = np.ones(N, np.float32)
    kw = dict(kernel=s["kernel"], optimizer=s["opt"], lr=s["lr"], alpha=s["alpha"], temperature=4.0, chol_a=float(g["chol_a"]), a_pre=float(g["a_pre"]),
              sigma_a=float(g["sigma"]), sigma_p=float(g["sigma"]))
    errs = {}
    c = _ctx(s, **kw)
    for k in range(K):  # score, phi: the reference's costs / actions injected
        c.set_theta(g["theta_in"][k])
        c.set_prior(g["mu0"], mix)
        phi, gl, gp = c.svmpc_phi(g["costs"][k], g["actions"][k])
        for q, v in (("score", gl + gp), ("phi", phi)):
            errs["%s[%d]" % (q, k)] = (min(elemerr(v, g[q][k]), elemerr(v, g[q + "_f64"][k])), float(g["tol_" + q]))
    c.close()
    c = _ctx(s, **kw)  # the updated particles: K optimiser steps from the recorded draws (Adam's state carried from step to step)
    c.set_theta(g["theta0"]); c.set_prior(g["mu0"], mix); c.set_a_mat(g["theta0"])
    for k in range(K):
        c.svmpc_optimize(g["state"], 1, g["eps"][k][None], g["params"][k][None])
        assert c.tick_stats()["tick2"] == 0  # (a two-pass family: the launch-per-iteration path)
        for q, v in (("costs", c.get_costs()), ("theta_after", c.get_theta())):
            errs["%s[%d]" % (q, k)] = (min(elemerr(v, g[q][k]), elemerr(v, g[q + "_f64"][k])), float(g["tol_" + q]))
    assert elemerr(g["costs_off"], g["costs"][-1]) >= 10 * float(g["tol_costs"]) and elemerr(g["costs_off"], c.get_costs()) >= 9 * float(g["tol_costs"])
    c.close()
    c = _ctx(s, **kw)  # forward(): the state the reference was in before it - its particles, prior, last costs
    c.set_theta(g["theta_in"][K - 1]); c.set_prior(g["mu0"], mix); c.set_a_mat(g["a_mat"][K - 2] if K > 1 else g["theta0"])
    c.likelihood_sample(g["state"], g["eps"][K - 1], g["params"][K - 1])
    c.set_theta(g["theta_after"][K - 1])
    a_seq, pw = c.svmpc_forward()
    ll, lp = c.get_log_weights()
    for q, v in (("log_l", ll), ("log_p", lp), ("p_weights", pw)):
        errs[q] = (_err(v, g, q), float(g["tol_" + q]))
    assert int(np.argmax(pw)) == int(np.argmax(g["p_weights"]))
    assert np.array_equal(a_seq, g["a_seq"])
    assert relerr(c.get_theta(), g["theta_rolled"]) < 1e-6  # (the roll and the prior refresh: test_forward_vs_reference's bounds)
    means, probs = c.get_prior()
    assert relerr(means, g["prior_means"]) < 1e-6 and elemerr(probs, g["prior_probs"]) < TOL
    c.close()
    print(name + " " + "  ".join("%s %.1e/%.1e" % (q, e, t) for q, (e, t) in errs.items()))
    for q, (e, t) in errs.items():
        assert e < t, (name, q, e, t)


# ------------------------------------------------------------------------------------------------ 3. device Philox noise
def host_costs(state, actions, params, up, fixed, log=False):
    """costs [S, N] of the actions [S, N, H, 1] replayed through the host CartPoleModel.step + QuadraticCost in torch, mean over the M rows"""
    from dust_amd.costs import QuadraticCost
    from dust_amd.models import CartPoleModel

    S, N, H = actions.shape[:3]
    model = CartPoleModel(dt=DT, uncertain_params=up, **fixed)
    cost = QuadraticCost(GOAL, W_STATE, W_TERM, W_CTRL)
    acts = torch.from_numpy(actions).reshape(S * N, H, 1)
    out = []
    for row in params:
        p = torch.from_numpy(np.asarray(row, np.float32)).reshape(1, -1)
        pd = model.params_to_dict((p.exp() if log else p).expand(S * N, -1))
        x = torch.from_numpy(np.asarray(state, np.float32)).expand(S * N, -1).clone()
        tot = torch.zeros(S * N)
        for t in range(H):
            tot = tot + cost.inst_cost(x, acts[:, t])
            x = model.step(x, acts[:, t], pd)
        out.append(tot + cost.term_cost(x))
    return torch.stack(out).mean(0).reshape(S, N).numpy()


def test_device_noise_costs_replay_through_the_host_model(golden):
    """One tick's rollouts at N 37, S 9, H 12, M 2 with the policy noise drawn on the device: the actions it used, fetched, replayed
    through the host model (bit-equal to the reference's step: tests/test_cartpole_cpu.py) - costs to 1e-5 (the reference's own d on
    these rollouts is 3e-7); the draws are standard normal; a clone continues identically."""
    s = dict(ROLLOUT_BY_TAG["ragged"], N=37, S=9, H=12, M=2)
    rng = np.random.default_rng(7)
    N, S, H, M = 37, 9, 12, 2
    mu = (0.4 * rng.standard_normal((N, H, 1))).astype(np.float32)
    th = (mu + 0.3 * rng.standard_normal((N, H, 1))).astype(np.float32)
    params = np.stack([rng.uniform(s["lo"], s["hi"], (M, 2)) for _ in range(2)]).astype(np.float32)
    state = golden("cartpole_ragged")["state"]
    c = _ctx(s, kernel="K1", lr=0.05, seed=9)
    c.set_theta(th); c.set_prior(mu); c.set_a_mat(th)
    cc = c.clone()
    costs, actions = c.likelihood_sample(state, None, params[0], want_actions=True)
    ref = host_costs(state, actions, params[0], s["up"], s["fixed"])
    e = elemerr(costs, ref)
    print("device noise: costs vs host replay %.1e" % e)
    assert e < TOL
    z = (actions - th[None]) / np.float32(SIGMA_A)
    assert abs(float(z.mean())) < 0.06 and abs(float(z.std()) - 1.0) < 0.06 and (np.abs(actions) > 1).mean() > 0.05
    a1, p1 = c.svmpc_tick(state, 2, params=params)
    cc.likelihood_sample(state, None, params[0])  # (the same stream position as c)
    a2, p2 = cc.svmpc_tick(state, 2, params=params)
    assert np.isfinite(a1).all() and abs(float(p1.sum()) - 1.0) < 1e-4
    assert np.array_equal(a1, a2) and np.array_equal(p1, p2)
    assert c.tick_stats()["tick2"] == 0
    c.close(); cc.close()


# ------------------------------------------------------------------------------------------------ 4. sharding
def test_cartpole_sharded_equals_unsharded(golden):
    """The family under particle sharding (2 and 4 sharded contexts in one process, all-gathers as slice copies): its rollout kernel takes
    (shard offset, local count) like every other kernel - the criterion of test_skid_steer_sharded_equals_unsharded."""
    from dust_amd.parallel import DeviceShard, LocalComm, tick

    s = dict(ROLLOUT_BY_TAG["ragged"], N=64, S=32, H=10, M=3)
    N, S, H, M, K, T = 64, 32, 10, 3, 2, 2
    rng = np.random.default_rng(5)
    mu = (0.4 * rng.standard_normal((N, H, 1))).astype(np.float32)
    th = (mu + 0.3 * rng.standard_normal((N, H, 1))).astype(np.float32)
    state = golden("cartpole_ragged")["state"]
    eps = rng.standard_normal((T, K, S, N, H, 1)).astype(np.float32)
    params = np.stack([[rng.uniform(s["lo"], s["hi"], (M, 2)) for _ in range(K)] for _ in range(T)]).astype(np.float32)
    kw = controller_kwargs(s, kernel="K1", lr=0.05, seed=11)
    ref = _ctx(s, kernel="K1", lr=0.05, seed=11)
    ref.set_theta(th); ref.set_prior(mu); ref.set_a_mat(th)
    outs = [ref.svmpc_tick(state, K, eps[t], params[t]) for t in range(T)]
    rt = ref.get_theta()
    assert not np.array_equal(rt, th)
    for world in (2, 4):
        shards = tuple(DeviceShard(dict(kw), r, world) for r in range(world))
        for sh in shards:
            sh.set_state(th, mu, th)
        for t in range(T):
            a_seq, pw = tick(shards, LocalComm(), state, K, eps[t], params[t], want_outputs=True, final_gather=(world == 2))
            assert np.array_equal(a_seq, outs[t][0]), (world, t)
            assert relerr(pw, outs[t][1]) < 1e-5
        for sh in shards:
            sh.sync()
            assert elemerr(sh.ctx.get_theta(), rt) < 2e-6, (world, sh.rank)
            sh.ctx.close()
    ref.close()


# ------------------------------------------------------------------------------------------------ 5. the filter: fixtures x forms
def _mpf(s, x0, obs0, **kw):
    from dust_amd import MpfContext

    return MpfContext(x0, obs0, lr=s["lr"], init_bw=s["bw"], optimizer=s["opt"], **model_kwargs(s), **kw)


@pytest.mark.parametrize("name", NAMES)
def test_filter_phi_vs_reference(golden, name):
    """dust_mpf_phi against the reference's MPF.phi; the fixture's power: with its branch ignored the reference itself is >= 10
    tolerances away."""
    g, s = golden("mpf_cartpole_" + name), BY_TAG[name]
    m = _mpf(s, g["x0"], g["obs0"])
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
def test_filter_optimize_vs_reference(golden, name, form, monkeypatch):
    """A two-step optimize() and two full calls (optimiser state carried over), in every form, against the reference's MPF.optimize;
    then the resulting prior's log-density at the probe points."""
    g, s = golden("mpf_cartpole_" + name), BY_TAG[name]
    Mp, bw, n = int(g["Mp"]), float(g["bw"]), int(g["n_steps"])
    _set_form(monkeypatch, form, Mp)
    m = _mpf(s, g["x0"], g["obs0"])
    gn = m.optimize(g["action"], g["obs1"], bw, 2)
    x2 = m.get_particles()
    _served(m, form, 1)
    m.close()
    errs = dict(disp_2=mpf_size_disp_err(x2, g), x_2=mpf_size_err(x2, g, "x_2"), grad_norms_2=mpf_size_err(gn, g, "grad_norms_2"))
    m = _mpf(s, g["x0"], g["obs0"])
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


SWEEP = [(Mp, f) for Mp in SWEEP_SIZES for f in FORMS if f == "single" or Mp >= 8]


@pytest.mark.parametrize("Mp,form", SWEEP, ids=["%d-%s" % c for c in SWEEP])
def test_filter_size_sweep_vs_reference(golden, Mp, form, monkeypatch):
    """P = 3 in log space at every edge of the launch geometry: a two-step optimize() in every eligible form - and the bare phi in the
    one-workgroup form - against the reference, x0 rebuilt from the seeded function the generator used."""
    g, s = golden("mpf_cartpole_sweep"), sweep_scenario(Mp)
    x0 = particles(s["up"], Mp, s["log"], s["seed"], s["spread"], s["centre"])
    q = lambda k: g["%s_%d" % (k, Mp)]
    _set_form(monkeypatch, form, Mp)
    m = _mpf(s, x0, g["obs0"])
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


# ------------------------------------------------------------------------------------------------ 6. the dual loop
def _plant(st, a):
    """the plant: the host CartPoleModel with other parameters than any filter starts from"""
    from dust_amd.models import CartPoleModel

    nxt = CartPoleModel(dt=DT, **TRUE).step(torch.from_numpy(np.asarray(st, np.float32)).reshape(1, 4), torch.from_numpy(np.asarray(a, np.float32)).reshape(1, 1))
    return nxt.reshape(-1).numpy()


def test_dual_tick_on_cartpole_equals_its_pieces():
    """dust_dual_tick with a cart-pole controller and filter that name the same uncertain parameters: the filter update with Silverman's
    bandwidth on the device, the controller's dynamics samples drawn from the refreshed prior on the device, the control tick - one call
    - against the same pieces called one by one with the same Philox key: bit-identical over three control periods.  A controller that
    names other parameters than the filter, or the same in another order, is refused."""
    from dust_amd import Context, MpfContext, _lib

    N, S, M, H, K, Mp = 32, 16, 3, 8, 2, 130
    rng = np.random.default_rng(11)
    mu = (0.4 * rng.standard_normal((N, H, 1))).astype(np.float32)
    th = (mu + 0.3 * rng.standard_normal((N, H, 1))).astype(np.float32)
    x0 = particles(P3, Mp, True, 77, 0.2)
    s0 = np.array([0.1, 0.2, 0.15, -0.1], np.float32)
    ckw = dict(model="cartpole", N=N, S=S, M=M, H=H, kernel="K1", lr=0.05, alpha=0.25, sigma_a=SIGMA_A, sigma_p=SIGMA_A, params_log_space=True,
               goal=GOAL, w_quad_state=W_STATE, w_quad_term=W_TERM, w_quad_ctrl=W_CTRL, seed=5)

    def make():
        c = Context(uncertain_params=P3, **ckw)
        c.set_theta(th); c.set_prior(mu); c.set_a_mat(th)
        m = MpfContext(x0, s0, model="cartpole", uncertain_params=P3, log_space=True, obs_std=0.05, lr=1e-4, init_bw=0.3)
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
    for up in (P3[::-1], ("mass_cart", "length", "g")):  # another column order; another parameter
        cw = Context(uncertain_params=up, **ckw)
        with pytest.raises(_lib.DustError) as e:
            cw.dual_tick(ma, sa, None, K)
        assert e.value.status == _lib.ERR_INVALID
        cw.close()
    for o in (ca, cb, ma, mb):
        o.close()


@pytest.mark.parametrize("name", ("p4_log", "nondefault"))
def test_mirror_mpf_over_cartpole_reproduces_the_fixture(golden, name):
    """MPF(init, GaussianLikelihood(obs, std, CartPoleModel(...), log_space)): params_dict, uncertain_params and dt reach the device from
    the model object; a deep copy (dust_mpf_clone) carries the model."""
    from dust_amd.inference import MPF, GaussianLikelihood
    from dust_amd.models import CartPoleModel

    g, s = golden("mpf_cartpole_" + name), BY_TAG[name]
    model = CartPoleModel(dt=s["dt"], uncertain_params=s["up"], **s["fixed"])
    lik = GaussianLikelihood(torch.tensor(g["obs0"]), s["obs_std"], model, log_space=s["log"])
    mpf = MPF(torch.tensor(g["x0"]), lik, bw=s["bw"], bw_scale=1.0, optimizer_class=torch.optim.SGD, lr=s["lr"])
    lik.condition(torch.tensor(g["action"]).view(1, 1), torch.tensor(g["obs1"]))
    mpf._dev.condition(g["action"], g["obs1"])
    assert mpf_size_err(mpf.phi(s["bw"]).numpy(), g, "phi0") < float(g["tol_phi0"])
    mpf = MPF(torch.tensor(g["x0"]), GaussianLikelihood(torch.tensor(g["obs0"]), s["obs_std"], model, log_space=s["log"]), bw=s["bw"], bw_scale=1.0,
              optimizer_class=torch.optim.SGD, lr=s["lr"])
    gn, bw = mpf.optimize(torch.tensor(g["action"]).view(1, 1), torch.tensor(g["obs1"]), bw=s["bw"], n_steps=s["n"])
    assert bw == s["bw"]
    assert mpf_size_err(mpf.x.numpy(), g, "x_n") < float(g["tol_x_n"])
    assert mpf_size_err(gn.numpy(), g, "grad_norms") < float(g["tol_grad_norms"])
    twin = copy.deepcopy(mpf)
    gn, _ = mpf.optimize(torch.tensor(g["action2"]).view(1, 1), torch.tensor(g["obs2"]), bw=s["bw"], n_steps=s["n"])
    gt, _ = twin.optimize(torch.tensor(g["action2"]).view(1, 1), torch.tensor(g["obs2"]), bw=s["bw"], n_steps=s["n"])
    assert mpf_size_err(mpf.x.numpy(), g, "x_n2") < float(g["tol_x_n2"])
    assert mpf_size_err(gn.numpy(), g, "grad_norms2") < float(g["tol_grad_norms2"])
    assert torch.equal(mpf.x, twin.x) and torch.equal(gn, gt)
    assert mpf_size_err(mpf.prior.log_prob(torch.tensor(g["probe"])).numpy(), g, "probe_log_prob") < float(g["tol_probe_log_prob"])


def test_mirror_controller_over_cartpole_reproduces_the_fixture(golden):
    """MultiDISCO.forward over dust_amd.models.CartPoleModel with QuadraticCost and recorded draws: the model's seven parameters, its
    uncertain names and the cost reach the device from the objects."""
    from dust_amd.controllers import MultiDISCO
    from dust_amd.costs import QuadraticCost
    from dust_amd.models import CartPoleModel
    from helpers import RecordedDraws

    g, s = golden("cartpole_params_log"), ROLLOUT_BY_TAG["params_log"]
    model = CartPoleModel(dt=DT, uncertain_params=s["up"], **s["fixed"])
    cost = QuadraticCost(GOAL, W_STATE, W_TERM, W_CTRL)
    ctrl = MultiDISCO(observation_space=model.observation_space, action_space=model.action_space, hz_len=s["H"], action_samples=s["S"],
                      params_samples=s["M"], temperature=4.0, a_cov=SIGMA_A ** 2 * torch.eye(1), inst_cost_fn=cost.inst_cost, term_cost_fn=cost.term_cost,
                      params_sampling=True, n_policies=s["N"], params_log_space=True)
    ctrl.a_mat = torch.tensor(g["a_mat0"])
    ctrl.return_rollouts = True
    ctrl.draw_source = RecordedDraws(params=[g["params"]])
    pd = torch.distributions.Independent(torch.distributions.Normal(torch.zeros(4), torch.ones(4)), 1)  # (its draws are the recorded ones)
    costs, states, actions, omega, _ = ctrl.forward(torch.tensor(g["state"]), model, pd, ext_actions=torch.tensor(g["ext_actions"]))
    assert _err(costs.numpy(), g, "costs") < float(g["tol_costs"])
    assert _err(states.numpy(), g, "states") < float(g["tol_states"])
    assert _err(omega.numpy(), g, "omega") < float(g["tol_omega"])


def test_dual_svmpc_on_cartpole_fused_equals_unfused():
    """DualSVMPC over CartPoleModel, five control periods: fused (one C call per period) and unfused (the loop's own calls) give the same
    actions, weights and filter particles.  An explicit filter bandwidth and one SVGD iteration per tick, so that both draw the same
    dynamics samples (the unfused loop draws one set per iteration and evaluates Silverman's rule on the host)."""
    from dust_amd.controllers import DualSVMPC, MultiDISCO
    from dust_amd.costs import QuadraticCost
    from dust_amd.inference import MPF, SVMPC, ExponentiatedUtility, GaussianLikelihood, get_gmm
    from dust_amd.kernels import RBFKernel
    from dust_amd.models import CartPoleModel

    N, S, M, H, Mp = 16, 16, 3, 6, 130
    rng = np.random.default_rng(21)
    mu0 = torch.tensor((0.4 * rng.standard_normal((N, H, 1))).astype(np.float32))
    init_policies = mu0 + torch.tensor((0.3 * rng.standard_normal((N, H, 1))).astype(np.float32))
    x0 = torch.tensor(particles(P3, Mp, True, 78, 0.2))
    init_state = torch.tensor([0.1, 0.2, 0.15, -0.1])
    cost = QuadraticCost(GOAL, W_STATE, W_TERM, W_CTRL)
    cov = SIGMA_A ** 2 * torch.eye(1)

    def make(fused):
        model = CartPoleModel(uncertain_params=P3)
        ctrl = MultiDISCO(observation_space=model.observation_space, action_space=model.action_space, hz_len=H, action_samples=S, params_samples=M,
                          temperature=4.0, a_cov=cov, inst_cost_fn=cost.inst_cost, term_cost_fn=cost.term_cost, params_sampling=True,
                          n_policies=N, params_log_space=True, seed=5)
        ctrl.a_mat = init_policies.clone()
        ctrl.return_rollouts = False
        mpf = MPF(init_particles=x0.clone(), likelihood=GaussianLikelihood(initial_obs=init_state, obs_std=0.05, model=model, log_space=True),
                  optimizer_class=torch.optim.SGD, lr=1e-4, bw=0.3, bw_scale=1.0)
        sv = SVMPC(likelihood=ExponentiatedUtility(alpha=0.25, n_samples=S, controller=ctrl, model=model), init_particles=init_policies.clone(),
                   prior=get_gmm(mu0, torch.ones(N), cov), kernel=RBFKernel(), n_particles=N, bw_scale=1.0, n_steps=1,
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


# ------------------------------------------------------------------------------------------------ 7. refusals
def _raw_mpf_create(P=3, ctrl_noise=0):
    """dust_mpf_create for the cart-pole model WITHOUT the dust_mpf_set_cartpole call MpfContext adds; (status, handle)"""
    from dust_amd import _lib as L
    from dust_amd.backend import make_config

    c = L.MpfConfig()
    c.abi_version, c.device, c.n_particles, c.dim_p = L.ABI_VERSION, 0, 16, P
    c.model_cfg = make_config(model="cartpole", uncertain_params=P3[:P])
    c.model_cfg.ctrl_noise = ctrl_noise
    c.dim_s, c.dim_a, c.model = 4, 1, L.MODEL_CARTPOLE
    c.log_space, c.obs_std, c.lr, c.bw_scale, c.init_bw = 0, 0.05, 1e-6, 1.0, 0.1
    x = particles(P3[:P], 16, False, 5, 0.15)
    obs = np.zeros(4, np.float32)
    h = L.VP()
    st = L.load().dust_mpf_create(C.byref(c), x.ctypes.data_as(L.FP), obs.ctypes.data_as(L.FP), C.byref(h))
    return st, h


def test_filter_refusals():
    from dust_amd import MpfContext, _lib as L
    from dust_amd.backend import _cartpole_struct

    lib = L.load()
    st, h = _raw_mpf_create(ctrl_noise=1)  # ctrl_noise stays a Particle field
    assert st == L.ERR_UNSUPPORTED and not h.value
    st, h = _raw_mpf_create()
    assert st == L.OK
    act, obs, phi = np.array([0.6], np.float32), np.array([0.3, 0.5, 0.4, -0.8], np.float32), np.empty((16, 3), np.float32)
    assert lib.dust_mpf_condition(h, act.ctypes.data_as(L.FP), obs.ctypes.data_as(L.FP)) == L.OK
    # before dust_mpf_set_cartpole nothing is sampled: phi and optimize have no column to differentiate
    assert lib.dust_mpf_phi(h, 0.1, phi.ctypes.data_as(L.FP)) == L.ERR_STATE
    assert lib.dust_mpf_optimize(h, None, None, 0.1, 2, None) == L.ERR_STATE
    vals = dict(g=9.8, f_mag=10.0, mass_cart=1.0, mass_pole=0.1, length=1.0, mu_c=5e-4, mu_p=2e-6)
    g = _cartpole_struct(vals, ["mass_cart", "length"])
    assert lib.dust_mpf_set_cartpole(h, C.byref(g)) == L.OK
    assert lib.dust_mpf_phi(h, 0.1, phi.ctypes.data_as(L.FP)) == L.ERR_STATE  # two sampled columns do not cover dim_p = 3
    g.f_mag = L.Param(L.PARAM_SAMPLED, 3, 10.0)
    assert lib.dust_mpf_set_cartpole(h, C.byref(g)) == L.ERR_INVALID  # a sampled column outside dim_p
    g.f_mag = L.Param(L.PARAM_SAMPLED, 1, 10.0)
    assert lib.dust_mpf_set_cartpole(h, C.byref(g)) == L.ERR_INVALID  # a column named twice
    g.f_mag = L.Param(L.PARAM_SAMPLED, 2, 10.0)
    assert lib.dust_mpf_set_cartpole(h, C.byref(g)) == L.OK
    assert lib.dust_mpf_phi(h, 0.1, phi.ctypes.data_as(L.FP)) == L.OK and np.isfinite(phi).all()
    lib.dust_mpf_destroy(h)
    # through the wrapper: a P = 1 filter cannot take two sampled parameters
    m = MpfContext(particles(("length",), 16, False, 5, 0.15), np.zeros(4, np.float32), model="cartpole", uncertain_params=("length",))
    with pytest.raises(L.DustError) as e:
        m.set_cartpole(uncertain_params=("length", "mass_cart"))
    assert e.value.status == L.ERR_INVALID
    m.close()
    p = MpfContext(np.ones((4, 2), np.float32), np.array([3.0, 0.0], np.float32))
    with pytest.raises(L.DustError) as e:  # the pendulum's filter has no cart-pole model to set
        p.set_cartpole(uncertain_params=("length", "mass_cart"))
    assert e.value.status == L.ERR_STATE
    p.close()


def test_controller_refusals(golden):
    from dust_amd import Context, _lib as L
    from dust_amd.backend import _cartpole_struct, make_config

    lib = L.load()
    s = ROLLOUT_BY_TAG["params"]
    g = golden("cartpole_params")
    cfg = make_config(**controller_kwargs(s))
    cfg.cost = L.COST_PENDULUM_QUADCOS  # a non-quadratic cost
    h = L.VP()
    assert lib.dust_create(C.byref(cfg), C.byref(h)) == L.ERR_UNSUPPORTED and not h.value
    cfg = make_config(**controller_kwargs(s))
    cfg.dim_a = 2
    assert lib.dust_create(C.byref(cfg), C.byref(h)) == L.ERR_INVALID and not h.value
    c = Context(**controller_kwargs(s))
    vals = dict(s["fixed"])
    st = _cartpole_struct(vals, ["length", "g"])
    st.g = L.Param(L.PARAM_SAMPLED, 3, 9.8)
    assert lib.dust_set_cartpole(c._h, C.byref(st)) == L.ERR_INVALID  # a sampled column outside dim_p = 3
    st.g = L.Param(L.PARAM_SAMPLED, 0, 9.8)
    assert lib.dust_set_cartpole(c._h, C.byref(st)) == L.ERR_INVALID  # a column named twice
    c.set_a_mat(g["a_mat0"]); c.set_theta(g["a_mat0"])
    with pytest.raises(L.DustError) as e:  # binary16 storage
        c.likelihood_sample(g["state"], g["eps"].astype(np.float16), g["params"])
    assert e.value.status == L.ERR_UNSUPPORTED
    with pytest.raises(L.DustError) as e:
        c.disco_forward(g["state"], g["ext_actions"], params=g["params"], want_states=True, store_f16=True)
    assert e.value.status == L.ERR_UNSUPPORTED
    with pytest.raises(L.DustError) as e:  # closed-loop serving with sampled dynamics
        c.serve_start(2)
    assert e.value.status == L.ERR_UNSUPPORTED
    costs = c.likelihood_sample(g["state"], g["eps"], g["params"])  # (the context still works after the refusals)
    assert _err(costs, g, "costs") < float(g["tol_costs"])
    c.set_param_weights(np.array([0.5, 0.25, 0.25], np.float32))  # sigma-point weights
    with pytest.raises(L.DustError) as e:
        c.likelihood_sample(g["state"], g["eps"], g["params"])
    assert e.value.status == L.ERR_UNSUPPORTED
    c.close()
    p = Context(model="pendulum", N=4, S=4, M=1, H=4)
    with pytest.raises(L.DustError) as e:  # the pendulum's context has no cart-pole model to set
        p.set_cartpole()
    assert e.value.status == L.ERR_STATE
    p.close()
