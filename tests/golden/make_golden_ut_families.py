#!/usr/bin/env python3
"""Golden vectors of the reference's sigma-point controller ("DISCO" case: MultiDISCO(params_sampling=MerweScaledUTF(...)), disco.py:211-292
with the weighted costs of disco.py:312-323) on its CartPoleModel and SkidSteerRobot - MultiDISCO.forward rollouts (ut_cartpole_p*.npz,
ut_skid_p*.npz), whole SVMPC ticks (ut_*_tick.npz) - and of the sigma points of the filter's prior (ut_sigma_mpf_*.npz:
compute_sigma_points(prior.mean, prior.variance.diag()) after MPF.update_prior(bw), mpf.py:26-38, utf.py:93-123).

TEST INFRASTRUCTURE.  Run from the repo root:  python tests/golden/make_golden_ut_families.py [--dry] [tag ...]
Needs the reference (build container only); writes arrays and scalars only.  Scenarios are data in tests/ut_cases.py.

The reference is imported as make_golden_cartpole.py and the skid-steer generators import it: through the shim, the cart-pole's
name-mangled attribute set on the instance, the quadratic cost as callables - whose `inst` IGNORES its actions: the reference hands the
cost function S N pts H states and S N H actions (disco.py:306-309), so only an action-free instantaneous cost runs there at all.
MerweScaledUTF hard-codes float32 weights (utf.py:86-87); the float64 run sets `_MerweScaledUTF__loc_weights` on the instance (no
reference text is changed).  Its sigma points stay float32 in either run (utf.py:108-118).

Tolerances follow make_golden_mpf_sizes.py / make_golden_cartpole.py: per quantity d = max(elemerr(fp32, fp32 with every input moved one
ulp), elemerr(fp32, float64)), tol = max(1e-5, 2 d), stored, and a fixture over 5e-5 is refused.  alpha = 0.5 (weights (-3, ...) at
n = 1); a scenario over the cap there takes alpha = 1.0 (weights (0, 1 / 2n, ...)) - the table says which was used.
Power: `costs_off` weights the instantaneous part by w[m] instead of w[(m H + t) mod M]; `costs_mean` (one fixture per family) is the
plain mean over the sigma points; both from a torch restatement of disco.py:306-323 that is first asserted equal to the reference's
costs, both asserted >= 10 tol away.  The filter fixtures carry `points_nobw`, the points with bw^2 left out of the variance.
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import make_golden as mg  # noqa: E402  (installs the shim, imports the reference)
import make_golden_cartpole as gc  # noqa: E402  (ref_model, tolerances, moved)
import make_golden_mpf_sizes as ms  # noqa: E402  (_dtype, one_ulp, caps)

import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.distributions as dist  # noqa: E402
import torch.distributions.multivariate_normal as mvn_mod  # noqa: E402
from dust.models.skid_steer_robot import SkidSteerRobot  # noqa: E402
from dust.utils.utf import MerweScaledUTF  # noqa: E402

sys.path.insert(0, os.path.join(mg.ROOT, "tests"))
import cartpole_cases as cpc  # noqa: E402
import ut_cases as cases  # noqa: E402
from helpers import elemerr  # noqa: E402

CAP, TOL = ms.CAP, ms.TOL


class Cost:
    """inst(x, a) = sum w_state (x - goal)^2 - the actions are ignored -, term(x) = sum w_term (x - goal)^2, in the default dtype"""

    def __init__(self, f):
        self.goal, self.w_state, self.w_term = torch.tensor(f["goal"]), torch.tensor(f["w_state"]), torch.tensor(f["w_term"])

    def inst(self, states, actions=None, n_pol=1, debug=None):
        return (((states - self.goal) ** 2) * self.w_state).sum(-1)

    def term(self, states, n_pol=1, debug=None):
        return (((states - self.goal) ** 2) * self.w_term).sum(-1)


def ref_model(s):
    f = cases.FAMILY[s["family"]]
    if s["family"] == "cartpole":
        return gc.ref_model(f["defaults"], s["up"], dt=f["dt"])
    return SkidSteerRobot(delta_t=f["dt"], min_wheel_speed=torch.tensor(f["lo"], dtype=torch.float32),
                          max_wheel_speed=torch.tensor(f["hi"], dtype=torch.float32), uncertain_params=tuple(s["up"]), **f["defaults"])


def transform(n, alpha, dt):
    tf = MerweScaledUTF(n=n, alpha=alpha)
    if dt == torch.float64:
        tf._MerweScaledUTF__loc_weights = torch.tensor(cases.weights(n, alpha)[0], dtype=torch.float64)
    return tf


def controller(s, model, cost, tf):
    f = cases.FAMILY[s["family"]]
    return mg.MultiDISCO(model.observation_space, model.action_space, s["H"], s["N"], s["S"], temperature=f["temperature"], ctrl_penalty=1.0,
                         a_cov=f["sigma_a"] ** 2 * torch.eye(f["da"]), inst_cost_fn=cost.inst, term_cost_fn=cost.term, params_sampling=tf,
                         params_log_space=False)


class NoGradUtility(mg.ExponentiatedUtility):
    """The reference's likelihood with its `sample` run under torch.no_grad(): SkidSteerRobot.step clamps a chunk view in place
    (skid_steer_robot.py:94), which autograd refuses when the actions carry a graph - and SVMPC.phi never differentiates through the
    rollouts (its likelihood gradient is the analytic one, svmpc.py:46-54).  The same arithmetic, no graph."""

    def sample(self, theta, state, params_dist):
        with torch.no_grad():
            return super().sample(theta, state, params_dist)


def params_dist(inp, t):
    return dist.MultivariateNormal(t(inp["dist_mean"]), covariance_matrix=torch.diag(t(inp["dist_std"]) ** 2))


def by_sigma(states, s, pts):
    """the reference's [S pts, N, H + 1, ds] (rollout (s N + n) pts + k runs sigma point k, disco.py:257-264) -> [pts, S, N, H + 1, ds]"""
    return states.reshape(s["S"], s["N"], pts, s["H"] + 1, -1).permute(2, 0, 1, 3, 4).contiguous()


# ---------------------------------------------------------------------------------------------- MultiDISCO.forward
def rollout_inputs(s):
    f = cases.FAMILY[s["family"]]
    rng = np.random.default_rng(s["seed"])
    N, S, H, da = s["N"], s["S"], s["H"], f["da"]
    a_mat0 = (f["a_scale"] * rng.standard_normal((N, H, da))).astype(np.float32)
    eps = rng.standard_normal((S, N, H, da)).astype(np.float32)
    ext = a_mat0[None] + np.float32(f["sigma_a"]) * eps
    mean, std = cases.dist_of(s)
    return dict(state=np.array(f["state0"], np.float32), a_mat0=a_mat0, ext_actions=ext.astype(np.float32), dist_mean=mean, dist_std=std)


def ref_forward(s, inp, alpha, dt=torch.float32):
    with ms._dtype(dt):
        t = lambda a: torch.as_tensor(np.asarray(a, np.float32)).to(dt)
        model, cost, tf = ref_model(s), Cost(cases.FAMILY[s["family"]]), transform(len(s["up"]), alpha, dt)
        ctrl = controller(s, model, cost, tf)
        ctrl.a_mat = t(inp["a_mat0"]).clone()  # (forward updates it in place)
        pd = params_dist(inp, t)
        with torch.no_grad():
            costs, states, actions, omega, plp = ctrl.forward(t(inp["state"]), model, pd, ext_actions=t(inp["ext_actions"]))
            sp = tf.compute_sigma_points(pd.mean, pd.covariance_matrix).T
        return dict(costs=mg.npf(costs), states=mg.npf(by_sigma(states, s, tf.pts)), states_flat=states, omega=mg.npf(omega), a_mat1=mg.npf(ctrl.a_mat),
                    a_mix=mg.npf(ctrl.a_mix), params_log_p=mg.npf(plp), sigma_points=mg.npf(sp), loc_weights=mg.npf(tf.loc_weights))


def restated(s, states, w, how):
    """disco.py:306-323 on the reference's own states [S pts, N, H + 1, ds] in fp32 torch; how: "ref" (the reference's views), "off" (the
    instantaneous part weighted by w[m]), "mean" (plain mean over the sigma points)"""
    S, N, H, pts = s["S"], s["N"], s["H"], w.numel()
    cost = Cost(cases.FAMILY[s["family"]])
    inst = cost.inst(states[..., :-1, :].reshape(-1, states.shape[-1]))
    term = cost.term(states[..., -1, :].reshape(-1, states.shape[-1]))
    if how == "ref":
        return mg.npf(torch.matmul(inst.view(-1, pts), w).view(S, N, H).sum(-1) + torch.matmul(term.view(-1, pts), w).view(S, N))
    if how == "off":
        return mg.npf((inst.view(S * N, pts, H) * w.view(1, pts, 1)).sum((1, 2)).view(S, N) + torch.matmul(term.view(-1, pts), w).view(S, N))
    return mg.npf((inst.view(S * N, pts, H).sum(-1) + term.view(S * N, pts)).mean(1).view(S, N))


def run_rollout(s, write=True):
    inp = rollout_inputs(s)
    keys = ("state", "a_mat0", "ext_actions", "dist_mean", "dist_std")
    for alpha in (cases.ALPHA, 1.0):
        r32 = ref_forward(s, inp, alpha)
        rp = ref_forward(s, gc.moved(inp, 2000 + s["seed"], keys), alpha)
        r64 = ref_forward(s, inp, alpha, torch.float64)
        f = cases.FAMILY[s["family"]]
        g = dict(N=s["N"], S=s["S"], H=s["H"], M=2 * len(s["up"]) + 1, P=len(s["up"]), uncertain=",".join(s["up"]), family=s["family"], alpha=alpha,
                 a_seq0=np.zeros((s["H"], f["da"]), np.float32), sigma_points=r32["sigma_points"], loc_weights=r32["loc_weights"],
                 params_log_p=r32["params_log_p"], sigma_scale=cases.weights(len(s["up"]), alpha)[1], **inp)
        bad, row = gc.tolerances((r32, rp, r64), cases.ROLLOUT_QUANT, g)
        if not bad or alpha == 1.0:
            break
        print("%-12s over the cap at alpha %.1f (%s): alpha 1.0" % (s["tag"], alpha, "; ".join(bad)))
    if s["states"]:
        # the float64 twin of the states as its scaled difference from the fp32 states, in fp32: back to 1e-14 of a state
        delta = (g.pop("states_f64") - g["states"].astype(np.float64)) * cpc.TWIN_SCALE
        g["states_f64_delta32"] = delta.astype(np.float32)
        assert elemerr(cases.twin(g, "states"), r64["states"]) < 1e-13
    else:
        del g["states"], g["states_f64"]
    w = torch.as_tensor(r32["loc_weights"])
    on = restated(s, r32["states_flat"], w, "ref")
    assert elemerr(on, g["costs"]) < 2e-7, "the restatement is not the reference's cost"
    g["costs_off"] = restated(s, r32["states_flat"], w, "off")
    power = [elemerr(g["costs_off"], g["costs"])]
    if s["mean"]:
        g["costs_mean"] = restated(s, r32["states_flat"], w, "mean")
        power.append(elemerr(g["costs_mean"], g["costs"]))
    # the closed form of the issue (tests/ut_cases.py ut_costs) on the float64 states is the reference's float64 cost
    closed = cases.ut_costs(r64["states"], cases.weights(len(s["up"]), alpha)[0], f["goal"], f["w_state"], f["w_term"])
    assert elemerr(closed, r64["costs"]) < 1e-12, elemerr(closed, r64["costs"])
    print("%-12s alpha %.1f  power %s | %s" % (s["tag"], alpha, " ".join("%.2e" % p for p in power), "  ".join(row)))
    if not min(power) >= 10 * g["tol_costs"]:
        bad.append("power %.2e < 10 x tol_costs %.1e" % (min(power), g["tol_costs"]))
    assert not bad or not write, (s["tag"], bad)
    if bad:
        print("   FAILS:", "; ".join(bad))
    if write:
        np.savez_compressed(os.path.join(mg.OUT, "ut_" + s["tag"] + ".npz"), **g)


# ---------------------------------------------------------------------------------------------- SVMPC ticks
def tick_inputs(s):
    f = cases.FAMILY[s["family"]]
    rng = np.random.default_rng(s["seed"])
    N, S, H, K, da = s["N"], s["S"], s["H"], cpc.TICK_ITERS, f["da"]
    mu0 = (0.8 * f["a_scale"] * rng.standard_normal((N, H, da))).astype(np.float32)
    theta0 = (mu0 + 0.6 * f["a_scale"] * rng.standard_normal((N, H, da))).astype(np.float32)
    mean, std = cases.dist_of(s)
    return dict(state=np.array(f["state0"], np.float32), mu0=mu0, theta0=theta0, eps=rng.standard_normal((K, S, N, H, da)).astype(np.float32),
                dist_mean=mean, dist_std=std)


def ref_tick(s, inp, alpha_ut, dt=torch.float32):
    """TICK_ITERS SVGD iterations (K1, SGD) and forward() of the reference's SVMPC over a sigma-point controller, from recorded policy
    noise, every stage recorded (make_golden_cartpole.py ref_tick with the transform in place of sampled parameters)"""
    f = cases.FAMILY[s["family"]]
    N, S, H, K, da = s["N"], s["S"], s["H"], cpc.TICK_ITERS, f["da"]
    with ms._dtype(dt):
        t = lambda a: torch.as_tensor(np.asarray(a, np.float32)).to(dt)
        model, cost, tf = ref_model(s), Cost(f), transform(len(s["up"]), alpha_ut, dt)
        ctrl = controller(s, model, cost, tf)
        ctrl.a_mat = t(inp["theta0"]).clone()
        prior = mg.get_gmm(t(inp["mu0"]), torch.ones(N), f["sigma_a"] ** 2 * torch.eye(da))
        alpha = s["alpha"]
        lik = (NoGradUtility if s["family"] == "skid" else mg.ExponentiatedUtility)(alpha=alpha, n_samples=S, controller=ctrl, model=model)
        sv = mg.SVMPC(init_particles=t(inp["theta0"]).clone(), prior=prior, likelihood=lik, kernel=mg.ref_shim.RBFKernel(), n_particles=N, bw_scale=1.0,
                      n_steps=1, optimizer_class=torch.optim.SGD, lr=s["lr"])
        pd = params_dist(inp, t)
        feed = [t(e) for e in inp["eps"]]
        saved = mvn_mod._standard_normal

        def fed(shape, dtype, device):
            if tuple(shape) == (S, N, H, da):
                return feed.pop(0).to(dtype)
            return saved(shape, dtype, device)

        state = t(inp["state"])
        sigma = ctrl.a_dist.covariance_matrix.diag().sqrt()
        out = {k: [] for k in ("theta_in", "actions", "costs", "score", "phi", "theta_after", "a_mat")}
        mvn_mod._standard_normal = fed
        try:
            for k in range(K):
                out["theta_in"].append(mg.npf(sv.theta))
                x = sv.theta.detach().clone().requires_grad_(True)
                grad_pri = torch.autograd.grad(sv.prior.log_prob(x).sum(), x)[0]  # svmpc.py:38-41
                sv.optimize(state, pd, n_steps=1)
                costs, actions = lik.last_costs.detach(), lik.last_actions.detach()
                w = torch.stack([torch.softmax(-costs[:, i] * alpha, dim=0) for i in range(N)], 1)  # svmpc.py:49-54
                grad_lik = (w.unsqueeze(-1).unsqueeze(-1) * ((actions - x.detach()) / sigma ** 2)).sum(0)
                out["score"].append(mg.npf(grad_lik + grad_pri))
                out["actions"].append(mg.npf(actions))
                out["costs"].append(mg.npf(costs))
                out["phi"].append(mg.npf(-sv.theta.grad))
                out["theta_after"].append(mg.npf(sv.theta))
                out["a_mat"].append(mg.npf(ctrl.a_mat))
        finally:
            mvn_mod._standard_normal = saved
        assert not feed
        with torch.no_grad():
            out["log_l"] = mg.npf(lik.log_prob(lik.last_costs))
            out["log_p"] = mg.npf(sv.prior.log_prob(sv.theta))
        a_seq, pw = sv.forward(state, pd)
        out.update(p_weights=mg.npf(pw), a_seq=mg.npf(a_seq), theta_rolled=mg.npf(sv.theta),
                   prior_means=mg.npf(sv.prior.component_distribution.base_dist.loc), prior_probs=mg.npf(sv.prior.mixture_distribution.probs))
        for k in ("theta_in", "actions", "costs", "score", "phi", "theta_after", "a_mat"):
            out[k] = np.stack(out[k])
        out["sigma_points"] = mg.npf(tf.compute_sigma_points(pd.mean, pd.covariance_matrix).T)
        out["loc_weights"] = mg.npf(tf.loc_weights)
    return out


def run_tick(s, write=True):
    inp = tick_inputs(s)
    keys = ("state", "mu0", "theta0", "eps", "dist_mean", "dist_std")
    for alpha in (cases.ALPHA, 1.0):
        r32 = ref_tick(s, inp, alpha)
        rp = ref_tick(s, gc.moved(inp, 3000 + s["seed"], keys), alpha)
        r64 = ref_tick(s, inp, alpha, torch.float64)
        g = dict(N=s["N"], S=s["S"], H=s["H"], M=2 * len(s["up"]) + 1, P=len(s["up"]), K=cpc.TICK_ITERS, uncertain=",".join(s["up"]), family=s["family"],
                 alpha_ut=alpha, lr=s["lr"], alpha=s["alpha"], sigma_scale=cases.weights(len(s["up"]), alpha)[1], **inp)
        for q in ("theta_in", "actions", "a_mat", "a_seq", "theta_rolled", "prior_means", "prior_probs", "sigma_points", "loc_weights"):
            g[q] = r32[q]
        bad, row = gc.tolerances((r32, rp, r64), cpc.TICK_QUANT, g, per_slice=("costs", "score", "phi", "theta_after"))
        if not bad or alpha == 1.0:
            break
        print("%-13s over the cap at alpha %.1f (%s): alpha 1.0" % (s["tag"], alpha, "; ".join(bad)))
    assert int(np.argmax(r32["p_weights"])) == int(np.argmax(r64["p_weights"])) == int(np.argmax(rp["p_weights"]))
    srt = np.sort(r32["p_weights"])
    print("%-13s alpha %.1f  top weights %.3f %.3f | %s" % (s["tag"], alpha, srt[-1], srt[-2], "  ".join(row)))
    if not srt[-1] > 1.05 * srt[-2]:
        bad.append("the top weight is not separated: choose another seed")
    assert not bad or not write, (s["tag"], bad)
    if bad:
        print("   FAILS:", "; ".join(bad))
    if write:
        np.savez_compressed(os.path.join(mg.OUT, "ut_" + s["tag"] + ".npz"), **g)


# ---------------------------------------------------------------------------------------------- sigma points of the filter's prior
def ref_sigma(s, x, dt=torch.float32, bw=None):
    """compute_sigma_points(prior.mean, prior.variance.diag()) of MPF.update_prior(bw) (disco.py:240-251); bw = 0: the variance without bw^2"""
    with ms._dtype(dt):
        xt = torch.as_tensor(np.asarray(x, np.float32)).to(dt)
        lik = mg.GaussianLikelihood(initial_obs=torch.zeros(2), obs_std=0.1, model=mg.PendulumModel(uncertain_params=("length",)), log_space=False)
        f = mg.MPF(init_particles=xt.clone(), likelihood=lik, optimizer_class=torch.optim.SGD, lr=1e-3, bw=s["bw"], bw_scale=1.0)
        f.update_prior(s["bw"])
        tf = MerweScaledUTF(n=s["P"], alpha=cases.ALPHA)
        var = f.prior.variance if bw is None else f.prior.variance - s["bw"] ** 2
        mean = f.prior.mean
        if dt == torch.float64:  # (compute_sigma_points casts to fp32, utf.py:108-118: the float64 answer is its formula in float64)
            U = ((cases.weights(s["P"])[1]) * var).sqrt()
            pts = torch.cat([mean.view(1, -1), mean + torch.diag(U), mean - torch.diag(U)], 0)
            return mg.npf(pts)
        return mg.npf(tf.compute_sigma_points(mean, var.diag()).T)


def run_sigma(s, write=True):
    x = cases.sigma_particles(s)
    r32, rp, r64 = ref_sigma(s, x), ref_sigma(s, ms.one_ulp(x, 4000 + s["seed"])), ref_sigma(s, x, torch.float64)
    g = dict(Mp=s["Mp"], P=s["P"], bw=s["bw"], alpha=cases.ALPHA, sigma_scale=cases.weights(s["P"])[1], x=x)
    bad, row = gc.tolerances((dict(points=r32), dict(points=rp), dict(points=r64)), ("points",), g)
    g["points_nobw"] = ref_sigma(s, x, bw=0.0)
    power = elemerr(g["points_nobw"], g["points"])
    if s["Mp"] == 1:  # the variance is exactly bw^2
        assert np.allclose(np.abs(r32[1:s["P"] + 1] - r32[0]).max(1), np.sqrt(g["sigma_scale"]) * s["bw"], rtol=1e-6)
    print("sigma %-8s power %.2e | %s" % (s["tag"], power, "  ".join(row)))
    if not power >= 10 * g["tol_points"]:
        bad.append("power %.2e < 10 x tol_points %.1e" % (power, g["tol_points"]))
    assert not bad or not write, (s["tag"], bad)
    if bad:
        print("   FAILS:", "; ".join(bad))
    if write:
        np.savez_compressed(os.path.join(mg.OUT, "ut_sigma_mpf_" + s["tag"] + ".npz"), **g)


if __name__ == "__main__":
    dry = "--dry" in sys.argv[1:]  # print the tables, assert and write nothing
    only = set(sys.argv[1:]) - {"--dry"}
    for s in cases.ROLLOUTS:
        if not only or s["tag"] in only:
            run_rollout(s, write=not dry)
    for s in cases.TICKS:
        if not only or s["tag"] in only:
            run_tick(s, write=not dry)
    for s in cases.SIGMA_MPF:
        if not only or "sigma" in only or ("sigma_" + s["tag"]) in only:
            run_sigma(s, write=not dry)
