#!/usr/bin/env python3
"""Golden vectors of the reference's controller on its CartPoleModel (dust/models/cartpole.py): MultiDISCO.forward rollouts
(cartpole_<tag>.npz), whole SVMPC ticks (cartpole_tick_*.npz), the model's own `step` (cartpole_step.npz) and its float64 parameter
Jacobian by autograd (cartpole_jac.npz).

TEST INFRASTRUCTURE.  Run from the repo root:  python tests/golden/make_golden_cartpole.py [--dry] [tag ...]
Needs the reference (build container only); writes arrays and scalars only.

The reference's `step` reads `self.__params_dict`, which Python mangles to `_CartPoleModel__params_dict`; the base class stored the dict
as `_BaseModel__params_dict`.  `ref_model` sets that one attribute ON THE INSTANCE; no reference text is changed.

Scenarios are data in tests/cartpole_cases.py.  Tolerances follow make_golden_mpf_sizes.py (read its docstring): per recorded quantity
d = max(elemerr(fp32 run, fp32 run with every input entry moved one ulp), elemerr(fp32 run, float64 run)), tol = max(1e-5, 2 d), stored
next to the quantity's `_f64` twin and asserted <= 5e-5.  (A quantity recorded per SVGD iteration takes the largest d of its slices.)
Power: `costs_off` are the costs with one thing ignored (the scenario's `off`: the step's +-1 clamp, `mass = m_c + m_c`, one friction
term), from a torch restatement of the rollout that is first asserted equal to the reference's (states bit for bit, costs to an ulp);
elemerr(costs_off, costs) >= 10 tol_costs is asserted.  The scalar-event fixture carries `states_off` instead - every rollout on
params[m] instead of params[r % M]: with M = 3 prime and N S no multiple of it every (s, n) still meets each draw once, so the MEAN
cost over the draws does not see the interleave; the states of the single rollouts do.
The start state has x_d != 0: CartPoleModel's cart friction is mu_c sign(x_d), and a start at exactly 0 moved by one ulp turns the
first step's friction on - the reference's own answer to that move is 1e-3 of a state, far over the caps.
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import make_golden as mg  # noqa: E402  (installs the shim, imports the reference)
import make_golden_mpf_sizes as ms  # noqa: E402  (the rule's pieces: _dtype, one_ulp, caps)

import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.distributions.multivariate_normal as mvn_mod  # noqa: E402
from dust.models.cartpole import CartPoleModel  # noqa: E402

sys.path.insert(0, os.path.join(mg.ROOT, "tests"))
import cartpole_cases as cases  # noqa: E402
from helpers import elemerr  # noqa: E402

CAP, TOL = ms.CAP, ms.TOL


def ref_model(fixed, up=None, dt=cases.DT):
    m = CartPoleModel(dt=dt, uncertain_params=tuple(up) if up else None, **fixed)
    m._CartPoleModel__params_dict = m.params_dict  # the name-mangled attribute `step` reads (cartpole.py:151/156)
    return m


class QuadCost:
    """inst(x, a) = sum w_state (x - goal)^2 + sum w_ctrl a^2, term(x) = sum w_term (x - goal)^2 in the default dtype"""

    def __init__(self):
        self.goal, self.w_state = torch.tensor(cases.GOAL), torch.tensor(cases.W_STATE)
        self.w_term, self.w_ctrl = torch.tensor(cases.W_TERM), torch.tensor(cases.W_CTRL)

    def inst(self, states, actions=None, n_pol=1, debug=None):
        return (((states - self.goal) ** 2) * self.w_state).sum(-1) + ((actions ** 2) * self.w_ctrl).sum(-1)

    def term(self, states, n_pol=1, debug=None):
        return (((states - self.goal) ** 2) * self.w_term).sum(-1)


class FixedDist:
    """a params_dist that hands out recorded draws"""

    def __init__(self, draws, scalar):
        self.draws, self.i, self.event_shape = list(draws), 0, torch.Size([]) if scalar else torch.Size([draws[0].shape[-1]])

    def sample(self, shape):
        self.i += 1
        return self.draws[self.i - 1].clone()

    def log_prob(self, x):
        return torch.zeros(x.shape[0])


def draw_params(s, rng, n):
    """n sets of [M, P] raw samples (a scalar-event distribution: [M])"""
    if not s["up"]:
        return None
    M, P = s["M"], len(s["up"])
    if s["dist"] == "uniform":
        p = rng.uniform(s["lo"], s["hi"], (n, M, P))
    else:
        p = np.asarray(s["loc"]) + np.asarray(s["scale"]) * rng.standard_normal((n, M, P))
    return p.astype(np.float32)


def controller(s, model, cost):
    return mg.MultiDISCO(model.observation_space, model.action_space, s["H"], s["N"], s["S"], temperature=cases.TEMPERATURE,
                         ctrl_penalty=s.get("ctrl_penalty", 1.0),
                         a_cov=cases.SIGMA_A ** 2 * torch.eye(1), inst_cost_fn=cost.inst, term_cost_fn=cost.term, params_sampling=bool(s["up"]),
                         params_samples=s["M"], params_log_space=s["log"])


def pdist_of(s, params, t):
    if params is None:
        return None
    scalar = s["dist"] == "scalar"
    return FixedDist([t(p).reshape(-1) if scalar else t(p) for p in params], scalar)


# ---------------------------------------------------------------------------------------------- MultiDISCO.forward
def rollout_inputs(s):
    rng = np.random.default_rng(s["seed"])
    N, S, H = s["N"], s["S"], s["H"]
    a_mat0 = (0.5 * rng.standard_normal((N, H, 1))).astype(np.float32)
    eps = rng.standard_normal((S, N, H, 1)).astype(np.float32)
    ext = a_mat0[None] + np.float32(cases.SIGMA_A) * eps  # (the device forms theta + chol * eps in this order)
    inp = dict(state=np.array(cases.STATE0, np.float32), a_mat0=a_mat0, eps=eps, ext_actions=ext.astype(np.float32))
    p = draw_params(s, rng, 1)
    if p is not None:
        inp["params"] = p[0]
    # (a generator of its own: the draws above are those of the fixtures made before scenarios carried an a_seq0)
    inp["a_seq0"] = (0.3 * np.random.default_rng(7000 + s["seed"]).standard_normal((H, 1)) if s.get("a_seq") else np.zeros((H, 1))).astype(np.float32)
    return inp


def ref_forward(s, inp, dt=torch.float32):
    with ms._dtype(dt):
        t = lambda a: torch.as_tensor(np.asarray(a, np.float32)).to(dt)
        model, cost = ref_model(s["fixed"], s["up"]), QuadCost()
        ctrl = controller(s, model, cost)
        ctrl.a_mat = t(inp["a_mat0"]).clone()  # (forward updates it in place)
        ctrl.a_seq = t(inp["a_seq0"]).clone()
        pd = pdist_of(s, [inp["params"]] if "params" in inp else None, t)
        with torch.no_grad():
            costs, states, actions, omega, _ = ctrl.forward(t(inp["state"]), model, pd, ext_actions=t(inp["ext_actions"]))
        return dict(costs=mg.npf(costs), states=mg.npf(states), omega=mg.npf(omega), a_mat1=mg.npf(ctrl.a_mat), a_mix=mg.npf(ctrl.a_mix))


def restated(s, inp, off=None):
    """MultiDISCO._rollout + _compute_cost over CartPoleModel.step in fp32 torch, operation by operation; `off` ignores one thing.
    With ctrl_penalty != 1 the costs carry the control-regularisation term (disco.py:338-346) through inp["a_mat0"], the a_mat the call
    sees, and inp["a_seq0"] (absent: zeros); off = "areg" leaves it out.
    -> dict(costs [S, N], states [M, S, N, H + 1, 4])"""
    N, S, H, M = s["N"], s["S"], s["H"], s["M"]
    f = torch.from_numpy
    p = dict(s["fixed"])
    if s["up"]:
        raw = f(inp["params"])
        raw = raw.exp() if s["log"] else raw
        if s["dist"] == "scalar" and off != "interleave":
            rows = raw.reshape(-1).repeat(1, S * N).reshape(-1, 1)  # disco.py:177-179: rollout r takes params[r % M]
        else:
            rows = raw.reshape(M, -1).repeat(1, S * N).reshape(-1, raw.reshape(M, -1).shape[1])
        for i, k in enumerate(s["up"]):
            p[k] = rows[:, i].reshape(-1, 1)
    g, m_c, m_p, length, mu_c, mu_p, f_mag = (p[k] for k in cases.NAMES7)
    acts = f(inp["ext_actions"]).reshape(-1, H, 1).repeat(M, 1, 1)
    x = f(inp["state"]).expand(M * S * N, -1).clone()
    cost, tot, traj = QuadCost(), torch.zeros(M * S * N), [x]
    for t in range(H):
        a = acts[:, t]
        tot = tot + cost.inst(x, a)
        xx, x_d, th, th_d = x.chunk(4, dim=1)
        u = (a if off == "clamp" else torch.clamp(a, min=-1, max=1)) * f_mag
        mass = m_c + (m_p if off == "mass" else m_c)
        pm = m_p * length
        cf = (0.0 if off == "mu_c" else mu_c) * x_d.sign()
        pf = ((0.0 if off == "mu_p" else mu_p) * th_d) / pm
        fac = (u + pm * th.sin() * th_d ** 2 - cf) / mass
        num = g * th.sin() - th.cos() * fac - pf
        den = length * (4.0 / 3 - (m_p * th.cos() ** 2) / mass)
        th_dd = num / den
        x_dd = fac - pm * th_dd * torch.cos(th) / mass
        x = x + torch.cat([x_d, x_dd, th_d, th_dd], dim=1) * cases.DT
        traj.append(x)
    # (the reference sums the H instantaneous costs of a rollout in one .sum(-1); accumulated here step by step - equal within an ulp)
    costs = (tot + cost.term(x)).view(M, S, N).mean(0)
    a_reg = cases.TEMPERATURE * (1 - s.get("ctrl_penalty", 1.0))
    if a_reg != 0 and off != "areg":
        e = torch.add(f(inp["ext_actions"]), -(f(inp["a_seq0"]) if "a_seq0" in inp else torch.zeros(H, 1)))
        a_pre = torch.inverse(cases.SIGMA_A ** 2 * torch.eye(1))
        costs = costs + (a_reg * torch.tensordot(-e, f(inp["a_mat0"]) @ a_pre, dims=([-2, -1], [-2, -1]))).diagonal(dim1=-2, dim2=-1)
    return dict(costs=mg.npf(costs), states=mg.npf(torch.stack(traj, 1).view(M, S, N, H + 1, 4)))


def tolerances(runs, quant, g, per_slice=()):
    """runs = (fp32, fp32 from one-ulp-moved inputs, float64): fills g with the quantities, twins and tolerances; -> (bad, row)"""
    r32, rp, r64 = runs
    row, bad = [], []
    for q in quant:
        g[q], g[q + "_f64"] = r32[q], r64[q]
        if q in per_slice:
            dp = max(elemerr(a, b) for a, b in zip(rp[q], r32[q]))
            d = max(dp, max(elemerr(a, b) for a, b in zip(r32[q], r64[q])))
        else:
            dp = elemerr(rp[q], r32[q])
            d = max(dp, elemerr(r32[q], r64[q]))
        g["tol_" + q] = max(TOL, 2.0 * d)
        row.append("%s %.1e%s" % (q, g["tol_" + q], "" if g["tol_" + q] == TOL else " (ulp)" if d == dp else " (f64)"))
        if g["tol_" + q] > CAP:
            bad.append("%s %.1e > cap %.0e" % (q, g["tol_" + q], CAP))
    return bad, row


def moved(inp, seed, keys):
    out = dict(inp)
    for i, k in enumerate(keys):
        if k in inp:
            out[k] = ms.one_ulp(inp[k], seed + i)
    return out


def run_rollout(s, write=True):
    inp = rollout_inputs(s)
    r32 = ref_forward(s, inp)
    rp = ref_forward(s, moved(inp, 2000 + s["seed"], ("state", "a_mat0", "ext_actions", "params") + (("a_seq0",) if s.get("a_seq") else ())))
    r64 = ref_forward(s, inp, torch.float64)
    g = dict(N=s["N"], S=s["S"], H=s["H"], M=s["M"], uncertain=",".join(s["up"]), off=s["off"],
             clamped_fraction=np.float32((np.abs(inp["ext_actions"]) > 1).mean()), **inp)
    bad, row = tolerances((r32, rp, r64), cases.ROLLOUT_QUANT, g)
    # storage (the file's size): the float64 twin of the states as its scaled difference from the fp32 states in binary16, which
    # cases.twin() undoes to 1e-10 of a state - five orders below the smallest tolerance, which was measured before the rounding
    delta = (g.pop("states_f64") - g["states"].astype(np.float64)) * cases.TWIN_SCALE
    assert np.abs(delta).max() < 6e4, "the difference leaves binary16's range"
    g["states_f64_delta16"] = delta.astype(np.float16)
    assert elemerr(cases.twin(g, "states"), r64["states"]) < 1e-9
    lead = cases.lead_quantity(s)
    on = restated(s, inp)
    assert elemerr(on["costs"], g["costs"]) < 2e-7 and np.array_equal(on["states"], g["states"]), "the restatement is not the reference's rollout"
    g[lead + "_off"] = restated(s, inp, s["off"])[lead]
    power = elemerr(g[lead + "_off"], g[lead])
    print("%-12s power(%s) %.2e  clamped %.0f %%  max|th| %.2f | %s" % (s["tag"], s["off"], power, 100 * float(g["clamped_fraction"]),
                                                                      float(np.abs(g["states"][..., 2]).max()), "  ".join(row)))
    if not power >= 10 * g["tol_" + lead]:
        bad.append("power %.2e < 10 x tol_%s %.1e" % (power, lead, g["tol_" + lead]))
    assert not bad or not write, (s["tag"], bad)
    if bad:
        print("   FAILS:", "; ".join(bad))
    if write:
        np.savez_compressed(os.path.join(mg.OUT, "cartpole_" + s["tag"] + ".npz"), **g)


# ---------------------------------------------------------------------------------------------- SVMPC ticks
def tick_inputs(s):
    rng = np.random.default_rng(s["seed"])
    N, S, H, K = s["N"], s["S"], s["H"], cases.TICK_ITERS
    mu0 = (0.4 * rng.standard_normal((N, H, 1))).astype(np.float32)
    theta0 = (mu0 + 0.3 * rng.standard_normal((N, H, 1))).astype(np.float32)
    inp = dict(state=np.array(cases.STATE0, np.float32), mu0=mu0, theta0=theta0, eps=rng.standard_normal((K, S, N, H, 1)).astype(np.float32))
    inp["params"] = draw_params(s, rng, K)
    return inp


def ref_tick(s, inp, dt=torch.float32, off=None):
    """two SVGD iterations and forward() of the reference's SVMPC from recorded draws, every stage recorded"""
    N, S, H, K = s["N"], s["S"], s["H"], cases.TICK_ITERS
    with ms._dtype(dt):
        t = lambda a: torch.as_tensor(np.asarray(a, np.float32)).to(dt)
        model, cost = ref_model(s["fixed"], s["up"]), QuadCost()
        ctrl = controller(s, model, cost)
        ctrl.a_mat = t(inp["theta0"]).clone()
        prior = mg.get_gmm(t(inp["mu0"]), torch.ones(N), cases.SIGMA_A ** 2 * torch.eye(1))
        if s["kernel"] == "K1":
            kernel = mg.ref_shim.RBFKernel()
        else:
            kernel = mg.iid_mp(base_kernel=mg.RBF(bandwidth=-1), ctrl_dim=1, indep_controls=True)
        alpha = s["alpha"]
        lik = mg.ExponentiatedUtility(alpha=alpha, n_samples=S, controller=ctrl, model=model)
        sv = mg.SVMPC(init_particles=t(inp["theta0"]).clone(), prior=prior, likelihood=lik, kernel=kernel, n_particles=N, bw_scale=1.0, n_steps=1,
                      optimizer_class=torch.optim.SGD if s["opt"] == "SGD" else torch.optim.Adam, lr=s["lr"])
        pd = pdist_of(s, inp["params"], t)
        feed = [t(e) for e in inp["eps"]]
        saved = mvn_mod._standard_normal

        def fed(shape, dtype, device):
            if tuple(shape) == (S, N, H, 1):
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
        L = torch.linalg.cholesky(ctrl.a_dist.covariance_matrix)
        out.update(chol_a=float(L[0, 0]), a_pre=float(ctrl.a_pre[0, 0]), sigma=float(sigma[0]))
    return out


def run_tick(s, write=True):
    inp = tick_inputs(s)
    r32 = ref_tick(s, inp)
    rp = ref_tick(s, moved(inp, 3000 + s["seed"], ("state", "mu0", "theta0", "eps", "params")))
    r64 = ref_tick(s, inp, torch.float64)
    g = dict(N=s["N"], S=s["S"], H=s["H"], M=s["M"], K=cases.TICK_ITERS, uncertain=",".join(s["up"]), off=s["off"], kernel=s["kernel"], opt=s["opt"],
             lr=s["lr"], alpha=s["alpha"], chol_a=r32["chol_a"], a_pre=r32["a_pre"], sigma=r32["sigma"], **inp)
    for q in ("theta_in", "actions", "a_mat", "a_seq", "theta_rolled", "prior_means", "prior_probs"):
        g[q] = r32[q]
    bad, row = tolerances((r32, rp, r64), cases.TICK_QUANT, g, per_slice=("costs", "score", "phi", "theta_after"))
    assert int(np.argmax(r32["p_weights"])) == int(np.argmax(r64["p_weights"])) == int(np.argmax(rp["p_weights"]))
    srt = np.sort(r32["p_weights"])
    assert srt[-1] > 1.05 * srt[-2], "the top weight is not separated: choose another seed"
    # power: the last iteration's costs with one thing ignored
    K = cases.TICK_ITERS
    last = dict(state=inp["state"], ext_actions=r32["actions"][-1], params=inp["params"][-1], a_mat0=r32["a_mat"][K - 2] if K > 1 else inp["theta0"])
    on = restated(s, last)["costs"]
    assert elemerr(on, g["costs"][-1]) < 2e-7, elemerr(on, g["costs"][-1])
    g["costs_off"] = restated(s, last, s["off"])["costs"]
    power = elemerr(g["costs_off"], g["costs"][-1])
    print("%-13s power(%s) %.2e  top weights %.3f %.3f | %s" % (s["tag"], s["off"], power, srt[-1], srt[-2], "  ".join(row)))
    if not power >= 10 * g["tol_costs"]:
        bad.append("power %.2e < 10 x tol_costs %.1e" % (power, g["tol_costs"]))
    assert not bad or not write, (s["tag"], bad)
    if bad:
        print("   FAILS:", "; ".join(bad))
    if write:
        np.savez_compressed(os.path.join(mg.OUT, "cartpole_" + s["tag"] + ".npz"), **g)


# ---------------------------------------------------------------------------------------------- step and its Jacobian
def run_step(write=True):
    """CartPoleModel.step on random states, actions beyond +-1, all seven parameters per row, some x_d = 0"""
    rng = np.random.default_rng(51)
    n = 64
    states = (rng.standard_normal((n, 4)) * np.array([1.0, 1.5, 2.0, 3.0])).astype(np.float32)
    states[::5, 1] = 0.0
    actions = (1.2 * rng.standard_normal((n, 1))).astype(np.float32)
    centre = np.array([dict(cases.DEFAULTS, **cases.FRICTION)[k] for k in cases.NAMES7])
    params = (centre * np.exp(0.2 * rng.standard_normal((n, 7)))).astype(np.float32)
    m = ref_model(cases.DEFAULTS, cases.NAMES7)
    f = torch.from_numpy
    nxt = m.step(f(states), f(actions), m.params_to_dict(f(params)))
    nominal = ref_model(cases.DEFAULTS).step(f(states), f(actions), None)
    g = dict(states=states, actions=actions, params=params, next=mg.npf(nxt), next_nominal=mg.npf(nominal), dt=cases.DT)
    print("step: %d rows, %d with x_d = 0, %d actions beyond +-1" % (n, int((states[:, 1] == 0).sum()), int((np.abs(actions) > 1).sum())))
    if write:
        np.savez_compressed(os.path.join(mg.OUT, "cartpole_step.npz"), **g)


def run_jac(write=True):
    """d (x_d', th_d') / d (the seven parameters), float64 autograd through the reference's step, in linear and in log space; rows cover
    sign(x_d) = 0 and a clamped action"""
    rng = np.random.default_rng(52)
    n = 12
    with ms._dtype(torch.float64):
        states = rng.standard_normal((n, 4)) * np.array([1.0, 1.5, 2.0, 3.0])
        states[::4, 1] = 0.0
        actions = 0.6 * rng.standard_normal((n, 1))
        actions[1::3] = np.sign(actions[1::3]) * 1.7
        centre = np.array([dict(cases.DEFAULTS, **cases.FRICTION)[k] for k in cases.NAMES7])
        params = centre * np.exp(0.2 * rng.standard_normal((n, 7)))
        m = ref_model(cases.DEFAULTS, cases.NAMES7)
        jac = {}
        for log in (False, True):
            J = np.zeros((n, 2, 7))
            for i in range(n):
                th = torch.tensor(np.log(params[i]) if log else params[i]).view(1, 7).requires_grad_(True)
                nxt = m.step(torch.tensor(states[i]).view(1, 4), torch.tensor(actions[i]).view(1, 1), m.params_to_dict(th.exp() if log else th))
                for r, row in enumerate((1, 3)):
                    J[i, r] = mg.npf(torch.autograd.grad(nxt[0, row], th, retain_graph=True)[0]).reshape(-1)
                for row in (0, 2):
                    assert float(torch.autograd.grad(nxt[0, row], th, retain_graph=True, allow_unused=True)[0].abs().max()) == 0.0
            jac["jac_log" if log else "jac_lin"] = J
    g = dict(states=states, actions=actions, params=params, dt=cases.DT, **jac)
    print("jac: %d rows, %d with x_d = 0, %d clamped" % (n, int((states[:, 1] == 0).sum()), int((np.abs(actions) > 1).sum())))
    if write:
        np.savez_compressed(os.path.join(mg.OUT, "cartpole_jac.npz"), **g)


if __name__ == "__main__":
    dry = "--dry" in sys.argv[1:]  # print the tables, assert and write nothing (for choosing a scenario's inputs)
    only = set(sys.argv[1:]) - {"--dry"}
    for s in cases.ROLLOUTS:
        if not only or s["tag"] in only:
            run_rollout(s, write=not dry)
    for s in cases.TICKS:
        if not only or s["tag"] in only:
            run_tick(s, write=not dry)
    if not only or "step" in only:
        run_step(write=not dry)
    if not only or "jac" in only:
        run_jac(write=not dry)
