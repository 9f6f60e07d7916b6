#!/usr/bin/env python3
"""Golden vectors of the reference's MultiDISCO in closed loop (dust/controllers/disco.py:139-417): per case of tests/disco_cases.py
LOOP_IDS, four periods of the reference's own `forward` - its draws recorded: the controller's `a_dist` hands out eps = chol_a z for the
recorded standard normals z -, `step(strategy, steps)` and the reference plant under the environment's true parameter row
(disco_loop_<case>.npz).  Pendulum without parameters (the MPPI baseline) and over 5 sigma points (DISCO), four policies with
ctrl_penalty 0.4 and steps 2 under both strategies, Particle on the demo's map, skid-steer with sampled rows and over 7 sigma points,
cart-pole.

TEST INFRASTRUCTURE.  Run from the repo root:  python tests/golden/make_golden_disco_loop.py [--dry] [case ...]
Needs the reference (build container only); writes arrays and scalars only.  Cases are data in tests/disco_cases.py.

The reference is imported as make_golden_amppi.py imports it (the shim, its models and cost callables, the float64 sigma weights set on
the instance).  Set ON THE INSTANCE besides (no reference text is changed): `ctrl.a_dist`, an object whose `sample` returns the recorded
draws, and - for sampled parameters - a `params_dist` object whose `sample` returns the recorded rows.

Every fixture runs in fp32, in fp32 with every input moved one ulp, and in float64; per quantity and period d = max of the two distances,
tol = max(1e-5, 2 d) - make_golden_amppi.py's margin - stored as `tol_<q>` [T]; a fixture over 5e-5 is refused.  Asserted in either mode:
the float64 restatement of tests/disco_cases.py reproduces the float64 run to 1e-12.  Stored besides: the float64 twins `<q>_f64`, the
recorded actions and sigma points, and the `_off` variants of tests/disco_cases.py OFF (`<q>_off_<name>` [T, ...], restated per period from
the twin's own previous period), each of which must lie >= 5 tol from the true quantity in at least one period - a wrong form need not
show in every one: with one policy and "average" a_seq IS a_mat from the second period on, and the two eps bases coincide.
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import make_golden as mg  # noqa: E402  (installs the shim, imports the reference)
import make_golden_amppi as ga  # noqa: E402  (ref_model, transform)
import make_golden_cartpole as gc  # noqa: E402  (moved)
import make_golden_mpf_sizes as ms  # noqa: E402  (_dtype, caps)

import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.distributions as dist  # noqa: E402

sys.path.insert(0, os.path.join(mg.ROOT, "tests"))
import disco_cases as cases  # noqa: E402
from helpers import elemerr  # noqa: E402

CAP, TOL = ms.CAP, ms.TOL


class Recorded:
    """stands in for a torch distribution: `sample` returns the recorded tensor"""

    def __init__(self, value, event=None):
        self.value = value
        self.event_shape = torch.Size([]) if event is None else torch.Size([event])

    def sample(self, sample_shape=None):
        return self.value.clone()

    def log_prob(self, x):
        return torch.zeros(x.shape[0])


def ref_loop(case, inp, dt=torch.float32):
    f = cases.family(case)
    T = cases.LOOP_T
    with ms._dtype(dt), torch.no_grad():
        t = lambda a: torch.as_tensor(np.asarray(a, np.float32)).to(dt)
        model, inst, term = ga.ref_model(case)
        tf = ga.transform(len(case["up"]), dt) if case["sigma"] else None
        a_cov = torch.as_tensor(cases.ac.a_cov_of(case)).to(dt)
        ctrl = mg.MultiDISCO(model.observation_space, model.action_space, case["H"], case["N"], case["S"], temperature=f["lam"],
                             ctrl_penalty=case["ctrl_penalty"], a_cov=a_cov,
                             inst_cost_fn=lambda x, a=None, n_pol=1, debug=None: inst(x, a) if case["family"] == "particle" else inst(x),
                             term_cost_fn=lambda x, n_pol=1, debug=None: term(x),
                             params_sampling=tf if tf is not None else (True if case["up"] else None), params_samples=case["M"],
                             params_log_space=False)
        ctrl.a_mat, ctrl.a_seq = t(inp["a_mat0"]).clone(), t(inp["a_seq0"]).clone()
        chol = a_cov.diag().sqrt()
        state = t(inp["state"])
        out = {k: [] for k in cases.LOOP_QUANT + ("actions",)}
        pd = None
        if tf is not None:
            pd = dist.MultivariateNormal(t(inp["dist_mean"]), covariance_matrix=torch.diag(t(inp["dist_std"]) ** 2))
            out["sigma_points"] = mg.npf(tf.compute_sigma_points(pd.mean, pd.covariance_matrix).T)
            out["loc_weights"] = mg.npf(tf.loc_weights)
        true = model.params_to_dict(t(inp["true"]).reshape(1, -1)) if "true" in inp else None
        for k in range(T):
            ctrl.a_dist = Recorded(chol * t(inp["z"][k]))
            if "params" in inp:
                pd = Recorded(t(inp["params"][k]), event=len(case["up"]))
            costs, _, actions, omega, _ = ctrl.forward(state, model, pd)
            acts = actions if actions.dim() == 4 else actions[0]
            out["actions"].append(mg.npf(acts))
            out["costs"].append(mg.npf(costs))
            out["omega"].append(mg.npf(omega))
            out["a_mat1"].append(mg.npf(ctrl.a_mat))
            out["a_mix"].append(mg.npf(ctrl.a_mix))
            nxt = ctrl.step(strategy=case["strategy"], steps=case["steps"]).clone()
            out["next"].append(mg.npf(nxt))
            out["a_seq"].append(mg.npf(ctrl.a_seq))
            out["a_mat"].append(mg.npf(ctrl.a_mat))
            state = model.step(state.view(1, -1), nxt[0].view(1, -1), true).view(-1)
            out["plant"].append(mg.npf(state))
        if case["family"] == "particle":
            out["grid"] = np.asarray(model.obst_map.map, np.float32)
    return {k: (np.stack(v) if isinstance(v, list) else v) for k, v in out.items()}


def run(case, write=True):
    inp = cases.loop_inputs(case)
    r32 = ref_loop(case, inp)
    rp = ref_loop(case, gc.moved(inp, 7000 + case["seed"], ("state", "a_mat0", "a_seq0", "z", "params", "dist_mean", "dist_std", "true")))
    r64 = ref_loop(case, inp, torch.float64)
    T = cases.LOOP_T
    g = dict(N=case["N"], S=case["S"], H=case["H"], M=case["M"], T=T, steps=case["steps"], strategy=case["strategy"], family=case["family"],
             ctrl_penalty=case["ctrl_penalty"], actions=r32["actions"], **inp)
    bad, row = [], []
    g["floor_next"] = np.sqrt((r64["a_mat1"].reshape(T, -1) ** 2).mean(1))  # (cases.loop_err: what a next action is held relative to)
    for q in cases.LOOP_QUANT:  # per-period tolerances
        g[q], g[q + "_f64"] = r32[q], r64[q]
        d = np.array([max(cases.loop_err(g, q, k, rp[q][k]), cases.loop_err(g, q, k, r32[q][k], r64[q][k])) for k in range(T)])
        g["tol_" + q] = np.maximum(TOL, 2.0 * d)
        row.append("%s %.1e" % (q, g["tol_" + q].max()))
        if g["tol_" + q].max() > CAP:
            bad.append("%s %.1e > cap" % (q, g["tol_" + q].max()))
    sp = None
    if case["sigma"]:
        g["sigma_points"], g["loc_weights"] = r32["sigma_points"], r32["loc_weights"]
        sp = r32["sigma_points"]
        assert np.array_equal(r64["sigma_points"].astype(np.float32), sp)  # (utf.py:108-118: fp32 in either run)
    if case["family"] == "particle":
        assert np.array_equal(cases.loop_grid(case), r32["grid"]), "oracle.grid_4x4_map is not the reference's map"
    re = cases.restate_loop(case, inp, sp)  # the restatement is the reference's float64 run
    for q in cases.LOOP_QUANT:
        e = elemerr(re[q], r64[q])
        assert e < 1e-12, (case["id"], q, e)
    power = []
    for name, v in cases.restate_off(case, inp, r64, sp).items():
        q = name.split("_off_")[0]
        g[name] = v.astype(np.float32)
        p = max(cases.loop_err(g, q, k, g[name][k]) / g["tol_" + q][k] for k in range(T))  # (the loop as a whole: some period shows it)
        power.append("%s %.0f" % (name.split("_off_")[1], p))
        if not p >= 5:
            bad.append("power(%s) %.1f tol < 5 tol" % (name, p))
    print("%-11s power %s | %s" % (case["id"], " ".join(power), "  ".join(row)))
    assert not bad or not write, (case["id"], bad)
    if bad:
        print("   FAILS:", "; ".join(bad))
    if write:
        np.savez_compressed(os.path.join(mg.OUT, "disco_loop_" + case["id"] + ".npz"), **g)
    return g


if __name__ == "__main__":
    # --dry: print the tables and write nothing; the fixture's conditions (cap, power) are reported, not asserted.  The restatement's
    # agreement with the float64 run is asserted in either mode: it is a check of tests/disco_cases.py, not of a fixture.
    dry = "--dry" in sys.argv[1:]
    only = set(sys.argv[1:]) - {"--dry"}
    for cid in cases.LOOP_IDS:
        if not only or cid in only:
            run(cases.BY_ID[cid], write=not dry)
