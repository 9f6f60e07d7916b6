#!/usr/bin/env python3
"""Golden vectors of the dual loop over the reference's AMPPI controller: its own `MPF.optimize` (dust/inference/mpf.py:64-86) and
`AMPPI.update_actions` (dust/controllers/amppi.py:227-260) composed as its simulation loop composes filter and controller
(dust/utils/simulations.py:104-138): model.params_dist = mpf.prior, update, plant step on a model with the true parameters, roll(1),
mpf.optimize(action, new_obs, bw, n_steps) - 4 periods (tests/golden/amppi_dual_<tag>.npz; scenarios in tests/amppi_dual_cases.py).

TEST INFRASTRUCTURE.  Run from the repo root:  python tests/golden/make_golden_amppi_dual.py [--dry] [tag ...]
Needs the reference (build container only); writes arrays and scalars only.

The reference is imported and fixed on the instance as make_golden_amppi.py and make_golden_mpf_sizes.py do (their builders are used).
Recorded inputs: the actions (a_seq + sigma_a z around the sequence the fp32 run had) and the parameter rows the reference's prior drew
under a fixed torch seed per period; the other runs are fed both.  `params_stale`: rows drawn the same way from the prior as it stood
BEFORE the filter update that opened the period.  Tolerances per period as make_golden_cartpole.tolerances: fp32, fp32 with every input one
ulp away, float64; tol = max(1e-5, 2 d); over the cap the fixture is refused (pick another seed).  Conditions asserted: top weight <= 0.5,
the update moves a_seq by >= 100 tol, every filter update moves the particles by >= 100 tol, each power variant (costs_disco, costs_noctrl,
costs_single, costs_stale) >= 10 tol from the truth, the controller half restated in float64 (amppi_cases.restate) equal to the float64
run to 1e-12."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import make_golden as mg  # noqa: E402
import make_golden_amppi as ga  # noqa: E402  (controller, ref_model, feed)
import make_golden_cartpole as gc  # noqa: E402  (moved)
import make_golden_mpf_sizes as ms  # noqa: E402  (_dtype, _filter)

import numpy as np  # noqa: E402
import torch  # noqa: E402

sys.path.insert(0, os.path.join(mg.ROOT, "tests"))
import amppi_cases as ac  # noqa: E402
import amppi_dual_cases as cases  # noqa: E402
from helpers import elemerr  # noqa: E402

TRUE = cases.TRUE


def _plant(s):
    if s["family"] in ("cartpole", "skid"):
        return ga.ref_model(dict(s, up=()))[0]
    if s["family"] == "pendulum":
        return mg.PendulumModel(**TRUE["pendulum"])
    return mg.Particle(**ac.PART_ENV, mass=TRUE["particle"]["mass"])


def ref_loop(s, inp, rec=None, dt=torch.float32):
    """rec None: actions are formed and rows drawn here (fp32 run) and returned; otherwise both are fed"""
    f, flt = ac.FAMILY[s["family"]], cases.FILTER[s["family"]]
    ms_s = dict(kind=s["family"], up=s["up"], log=False, obs_std=flt["obs_std"], opt="SGD", lr=flt["lr"], bw=s["bw"] if s["bw"] else 0.1)
    with ms._dtype(dt):
        t = lambda a: torch.as_tensor(np.asarray(a, np.float32)).to(dt)
        ctrl, model, tf = ga.controller(s, dt)
        plant = _plant(s)
        if s["family"] in ("cartpole", "skid"):
            lik = mg.GaussianLikelihood(initial_obs=t(inp["state"]), obs_std=flt["obs_std"], model=ga.ref_model(s)[0], log_space=False)
            mpf = mg.MPF(init_particles=t(inp["x0"]).clone(), likelihood=lik, optimizer_class=torch.optim.SGD, lr=flt["lr"], bw=s["bw"], bw_scale=1.0)
        else:
            mpf, _ = ms._filter(ms_s, t(inp["x0"]), t(inp["state"]))
        ctrl.a_seq = t(inp["a_seq0"]).clone()
        state = t(inp["state"])
        out = {k: [] for k in cases.QUANT + ("plant", "actions") + (("sigma_points",) if tf is not None else ("params", "params_stale"))}

        def draw(k):
            if rec is not None:
                return None
            torch.manual_seed(1000 * s["seed"] + k)
            model.params_dist = mpf.prior
            return mg.npf(model.dict_to_params(type(model).sample_params(model, 1 if s["mode"] == "single" else s["S"]))).astype(np.float32)

        stale = np.zeros((1 if s["mode"] == "single" else s["S"], len(s["up"])), np.float32)
        for k in range(cases.TICKS):
            model.__dict__.pop("sample_params", None)
            rows = None if tf is not None else (rec["params"][k] if rec is not None else draw(k))
            a = rec["actions"][k] if rec is not None else (mg.npf(ctrl.a_seq)[None] + np.float32(f["sigma_a"]) * inp["z"][k]).astype(np.float32)
            if tf is not None:  # the sigma points of the filter's prior (amppi.py:164-175 reads params_dist.mean / .variance)
                model.params_dist = mpf.prior
                model.to_params_dict = model.params_to_dict
                out["sigma_points"].append(mg.npf(tf.compute_sigma_points(mpf.prior.mean, mpf.prior.variance.diag()).T).astype(np.float32))
            else:
                ga.feed(model, rows, t)
            with torch.no_grad():
                costs, _, _, omega = ctrl.update_actions(model, state, t(a))
            a0 = ctrl.a_seq[0].clone()
            out["actions"].append(a)
            if tf is None:
                out["params"].append(rows); out["params_stale"].append(rec["params_stale"][k] if rec is not None else stale)
            out["costs"].append(mg.npf(costs)); out["omega"].append(mg.npf(omega)); out["a_seq1"].append(mg.npf(ctrl.a_seq))
            with torch.no_grad():
                state = (plant.step(state.view(1, -1), a0.view(1, -1), None) if s["family"] in ("skid", "cartpole") else
                         plant.step(state.view(1, -1), a0.view(1, -1))).view(-1)
            out["plant"].append(mg.npf(state))
            ctrl.roll(1)
            model.__dict__.pop("sample_params", None)
            stale = draw(k + 1) if rec is None and tf is None else None  # (the prior before this period's filter update, under the NEXT period's seed)
            _, bw = mpf.optimize(a0.reshape(()) if s["family"] == "pendulum" else (a0.view(1, -1) if s["family"] == "skid" else a0), state, bw=s["bw"], n_steps=s["mpf_steps"])
            out["x"].append(mg.npf(mpf.x)); out["bw"].append(np.array([float(bw)]))
        return {k: np.stack(v) for k, v in out.items()}


def run(s, write=True):
    inp = cases.inputs(s)
    r32 = ref_loop(s, inp)
    rec = {k: r32[k] for k in ("actions", "params", "params_stale") if k in r32}
    mv = gc.moved(dict(inp, **rec), 7000 + s["seed"], ("state", "a_seq0", "x0", "actions", "params"))
    rp = ref_loop(s, mv, rec=mv)
    r64 = ref_loop(s, inp, rec=rec, dt=torch.float64)
    f = ac.FAMILY[s["family"]]
    g = dict(S=s["S"], H=s["H"], P=len(s["up"]), Mp=s["Mp"], T=cases.TICKS, mode=s["mode"], family=s["family"], uncertain=",".join(s["up"]), lam=f["lam"],
             mpf_steps=s["mpf_steps"], bw_in=-1.0 if s["bw"] is None else s["bw"], state=inp["state"], a_seq0=inp["a_seq0"], x0=inp["x0"], **rec)
    if s["mode"] == "ut":
        g["sigma_points"], g["loc_weights"] = r32["sigma_points"], np.asarray(ac.weights(len(s["up"]))[0], np.float32)
        g["sigma_scale"] = float(ac.weights(len(s["up"]))[1])
    bad, row = [], []
    for q in cases.QUANT + ("plant",) + (("sigma_points",) if s["mode"] == "ut" else ()):
        g[q], g[q + "_f64"] = r32[q].astype(np.float32), r64[q]
        d = np.array([max(elemerr(rp[q][k], r32[q][k]), elemerr(r32[q][k], r64[q][k])) for k in range(cases.TICKS)])
        g["tol_" + q] = np.maximum(cases.TOL, 2.0 * d)
        row.append("%s %s" % (q, " ".join("%.1e" % v for v in g["tol_" + q])))
        if g["tol_" + q].max() > cases.CAP:
            bad.append("%s %.1e > cap" % (q, g["tol_" + q].max()))
    top = float(np.exp(r32["omega"]).max())
    if not top <= 0.5:
        bad.append("top weight %.3f > 0.5" % top)
    prev_seq = [inp["a_seq0"]] + [np.concatenate([r32["a_seq1"][k][1:], np.zeros_like(inp["a_seq0"][:1])]) for k in range(cases.TICKS - 1)]
    prev_x = [inp["x0"]] + list(r32["x"][:-1])
    power = []
    for k in range(cases.TICKS):
        if not elemerr(r32["a_seq1"][k], prev_seq[k]) >= 100 * g["tol_a_seq1"][k]:
            bad.append("period %d: a_seq moves < 100 tol" % k)
        mx = elemerr(r32["x"][k], prev_x[k])
        if not mx >= 100 * g["tol_x"][k]:
            bad.append("period %d: particles move %.1e < 100 tol %.1e" % (k, mx, g["tol_x"][k]))
        e = elemerr(cases.restate_costs(s, g, k, None)["costs"], r64["costs"][k])  # the controller half IS the float64 run
        assert e < 1e-12, (s["tag"], k, e)
    for v in cases.variants_of(s):
        ks = range(1, cases.TICKS) if v == "stale" else range(cases.TICKS)
        g["costs_" + v] = np.stack([cases.restate_costs(s, g, k, v)["costs"].astype(np.float32) if k in ks else g["costs"][k] for k in range(cases.TICKS)])
        p = min(elemerr(g["costs_" + v][k], g["costs"][k]) / g["tol_costs"][k] for k in ks)
        power.append("%s %.0f tol" % (v, p))
        if not p >= 10:
            bad.append("power(%s) %.1f tol < 10 tol" % (v, p))
    print("%-10s top %.3f  power %s | %s" % (s["tag"], top, " ".join(power), "  ".join(row)))
    assert not bad or not write, (s["tag"], bad)
    if bad:
        print("   FAILS:", "; ".join(bad))
    if write:
        np.savez_compressed(os.path.join(mg.OUT, "amppi_dual_" + s["tag"] + ".npz"), **g)
    return g


if __name__ == "__main__":
    dry = "--dry" in sys.argv[1:]
    only = set(sys.argv[1:]) - {"--dry"}
    for s in cases.SCENARIOS:
        if not only or s["tag"] in only:
            run(s, write=not dry)
