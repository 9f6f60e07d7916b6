#!/usr/bin/env python3
"""Golden vectors of the reference's dynamics filter (dust/inference/mpf.py MPF + likelihoods.py GaussianLikelihood) on its
CartPoleModel (dust/models/cartpole.py): the columns of the one-step Jacobian that only autograd can vouch for.

TEST INFRASTRUCTURE.  Run from the repo root:  python tests/golden/make_golden_mpf_cartpole.py [--dry] [tag ...]
Needs the reference (build container only); writes tests/golden/mpf_cartpole_<tag>.npz and mpf_cartpole_sweep.npz (arrays and scalars only).
The model is made by make_golden_cartpole.ref_model, which sets the one name-mangled attribute the reference's step reads on the instance.

Scenarios, recorded quantities, `_f64` twins, tolerances, caps and power follow make_golden_mpf_sizes.py (read its docstring): per
quantity d = max(elemerr(fp32 run, fp32 run from x0 with every entry moved one ulp), elemerr(fp32 run, float64 run)), tol = max(1e-5,
2 d) <= 5e-5, tol_disp_2 <= 2e-3, elemerr(phi0_off, phi0) >= 10 tol_phi0 and >= 10 tol_disp_2.  The scenarios themselves are data in
tests/cartpole_cases.py, shared with the tests.  The action reaches `condition` as a [1, 1] tensor.

What `off` (-> phi0_off) ignores, per scenario:
  p3_lin / p4_log      log: the particles read in the other parameter space
  fric_log, p2_lm      detach: one column (mu_p / length) cut out of the likelihood's graph
  sat                  noclamp: the step's +-1 clamp of the action removed (action 1.7)
  xd_zero              obs0: x_d = 0.4 instead of 0 (with x_d = 0 the mu_c column of the likelihood vanishes: sign(0) = 0)
  p2_ml                up: the columns read in the other order
  p1_length_600, ragged_1021   drop_last: the last particle left out (a key loop that stops short)
  nondefault           defaults: the constructor's fixed parameters and dt instead of the scenario's
  adam_130             action: half the action (the scenario is about Adam's state across calls)

mpf_cartpole_sweep.npz: P = 3 in log space at every edge of the launch geometry (tests/mpf_skid_cases.py SWEEP_SIZES); per size n the
keys phi0_n, x_2_n, grad_norms_2_n, their _f64 twins (stored in fp32; x_2's as the displacement disp_2_f64_n) and tol_*_n / tol_disp_2_n
under the same rule; x0 is rebuilt by the tests from cartpole_cases.particles, not stored.
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import make_golden as mg  # noqa: E402  (installs the shim, imports the reference)
import make_golden_mpf_sizes as ms  # noqa: E402  (the rule's pieces: _DetachedColumns, _dtype, one_ulp, QUANT, caps)

import numpy as np  # noqa: E402
import torch  # noqa: E402
import dust.models.cartpole as cartpole_mod  # noqa: E402
import make_golden_cartpole as mc  # noqa: E402  (ref_model)

sys.path.insert(0, os.path.join(mg.ROOT, "tests"))
import cartpole_cases as cases  # noqa: E402
from helpers import elemerr  # noqa: E402

CAP, CAP_DISP, TOL = ms.CAP, ms.CAP_DISP, ms.TOL
SWEEP_QUANT = ("phi0", "x_2", "grad_norms_2")


class _NoClamp:
    """`torch` as dust.models.cartpole sees it, with clamp the identity"""

    def __getattr__(self, k):
        return getattr(torch, k)

    @staticmethod
    def clamp(x, **kw):
        return x


def _model(s, up=None, true=False, **over):
    if true:
        return mc.ref_model(cases.TRUE, None, s["dt"])
    return mc.ref_model(over.get("fixed", s["fixed"]), s["up"] if up is None else up, over.get("dt", s["dt"]))


def _step_true(s, obs, act):
    return _model(s, true=True).step(obs.view(1, -1), act.view(1, -1), None).view(-1).detach()


def make_inputs(s):
    x0 = cases.particles(s["up"], s["Mp"], s["log"], s["seed"], s["spread"], s["centre"])
    obs0, action = torch.tensor(s["obs0"]), torch.tensor(s["action"])
    obs1 = _step_true(s, obs0, action)
    action2 = action * 0.5
    obs2 = _step_true(s, obs1, action2)
    return dict(x0=x0, obs0=mg.npf(obs0), action=mg.npf(action), obs1=mg.npf(obs1), action2=mg.npf(action2), obs2=mg.npf(obs2))


def _filter(s, x0, obs0, **off):
    if off.get("defaults"):
        model = _model(s, dt=cases.DT, fixed=cases.DEFAULTS)
    else:
        model = _model(s, up=off.get("up"))
    kw = dict(initial_obs=obs0, obs_std=s["obs_std"], model=model, log_space=off.get("log", s["log"]))
    lik = ms._DetachedColumns(off["detach"], **kw) if off.get("detach") else mg.GaussianLikelihood(**kw)
    if s["opt"] == "Adam":
        f = mg.MPF(init_particles=x0.clone(), likelihood=lik, lr=s["lr"], bw=s["bw"], bw_scale=1.0)
        assert isinstance(f.optimizer, torch.optim.Adam)
    else:
        f = mg.MPF(init_particles=x0.clone(), likelihood=lik, optimizer_class=torch.optim.SGD, lr=s["lr"], bw=s["bw"], bw_scale=1.0)
    return f, lik


def ref_phi(s, inp, dt=torch.float32, x0=None, **off):
    with ms._dtype(dt):
        t = lambda a: torch.as_tensor(np.asarray(a, np.float32)).to(dt)
        f, lik = _filter(s, t(inp["x0"] if x0 is None else x0), t(off.get("obs0", inp["obs0"])), **{k: v for k, v in off.items() if k != "obs0"})
        lik.condition(t(off.get("action", inp["action"])).view(1, 1), t(inp["obs1"]))
        if off.get("noclamp"):
            cartpole_mod.torch = _NoClamp()
        try:
            return f.phi(s["bw"]).detach().cpu().numpy().copy()
        finally:
            cartpole_mod.torch = torch


def ref_run(s, inp, dt=torch.float32, x0=None, full=True):
    out = dict(phi0=ref_phi(s, inp, dt, x0))
    with ms._dtype(dt):
        t = lambda a: torch.as_tensor(np.asarray(a, np.float32)).to(dt)
        act = lambda a: t(a).view(1, 1)
        x = t(inp["x0"] if x0 is None else x0)
        f, _ = _filter(s, x, t(inp["obs0"]))
        gn, _ = f.optimize(act(inp["action"]), t(inp["obs1"]), bw=s["bw"], n_steps=2)
        out.update(x_2=mg.npf(f.x), grad_norms_2=mg.npf(gn))
        if not full:
            return out
        f, _ = _filter(s, x, t(inp["obs0"]))
        gn, _ = f.optimize(act(inp["action"]), t(inp["obs1"]), bw=s["bw"], n_steps=s["n"])
        out.update(x_n=mg.npf(f.x), grad_norms=mg.npf(gn))
        gn, _ = f.optimize(act(inp["action2"]), t(inp["obs2"]), bw=s["bw"], n_steps=s["n"])
        out.update(x_n2=mg.npf(f.x), grad_norms2=mg.npf(gn))
        lo, hi = float(inp["x0"].min()) - 0.5, float(inp["x0"].max()) + 0.5
        probe = torch.linspace(lo, hi, 7).view(-1, 1).expand(-1, x.shape[1]).contiguous().to(dt)
        out.update(probe=mg.npf(probe).astype(np.float32), probe_log_prob=mg.npf(f.prior.log_prob(probe)))
    return out


def tolerances(s, inp, quant, full):
    """the recorded quantities of one scenario with their _f64 twins and tolerances; (dict, list of cap violations, table row)"""
    r32 = ref_run(s, inp, full=full)
    rp = ref_run(s, inp, x0=ms.one_ulp(inp["x0"], 1000 + s["seed"]), full=full)
    r64 = ref_run(s, inp, torch.float64, full=full)
    g, row, bad = {}, [], []
    for q in quant:
        g[q], g[q + "_f64"] = r32[q], r64[q]
        dp = elemerr(rp[q], r32[q])
        d = max(dp, elemerr(r32[q], r64[q]))
        g["tol_" + q] = max(TOL, 2.0 * d)
        row.append("%s %.1e%s" % (q, g["tol_" + q], "" if g["tol_" + q] == TOL else " (ulp)" if d == dp else " (f64)"))
        if g["tol_" + q] > CAP:
            bad.append("%s %.1e > cap %.0e" % (q, g["tol_" + q], CAP))
    rms = lambda a: float(np.sqrt(np.mean(np.asarray(a, np.float64) ** 2)))
    g["tol_disp_2"] = g["tol_x_2"] * rms(r32["x_2"]) / rms(r32["x_2"].astype(np.float64) - inp["x0"])
    if g["tol_disp_2"] > CAP_DISP:
        bad.append("tol_disp_2 %.1e > cap %.0e" % (g["tol_disp_2"], CAP_DISP))
    if full:
        g["probe"] = r32["probe"]
    return g, bad, row


def run(s, write=True):
    tag = s["tag"]
    inp = make_inputs(s)
    q, bad, row = tolerances(s, inp, ms.QUANT, True)
    g = dict(Mp=s["Mp"], P=inp["x0"].shape[1], n_steps=s["n"], log_space=int(s["log"]), bw=s["bw"], lr=s["lr"], obs_std=s["obs_std"],
             model_kind="cartpole", optimizer=s["opt"], uncertain=",".join(s["up"]), fixed=np.array([s["fixed"][k] for k in cases.NAMES7]),
             dt=s["dt"], **inp, **q)
    off = dict(s["off"])
    if off.pop("drop_last", False):
        phi_off = ref_phi(s, inp, x0=inp["x0"][:-1])
        power = elemerr(phi_off, g["phi0"][:-1])
    else:
        phi_off = ref_phi(s, inp, **off)
        power = elemerr(phi_off, g["phi0"])
    g["phi0_off"] = phi_off
    moved = float(np.abs(g["x_n"].astype(np.float64) - inp["x0"]).max())
    print("%-13s Mp %4d  power %.2e  tol_disp_2 %.1e  max move %.3f | %s" % (tag, s["Mp"], power, g["tol_disp_2"], moved, "  ".join(row)))
    if not (power >= 10 * g["tol_phi0"] and power >= 10 * g["tol_disp_2"]):
        bad.append("power %.2e < 10 x (tol_phi0 %.1e, tol_disp_2 %.1e)" % (power, g["tol_phi0"], g["tol_disp_2"]))
    assert not bad or not write, (tag, bad, "change lr / bw / spread of the scenario, not the caps")
    if bad:
        print("   FAILS:", "; ".join(bad))
    assert all(np.isfinite(v).all() for v in g.values() if isinstance(v, np.ndarray))
    if write:
        np.savez_compressed(os.path.join(mg.OUT, "mpf_cartpole_" + tag + ".npz"), **g)
    return g


def run_sweep(write=True):
    g = dict(sizes=np.array(cases.SWEEP_SIZES))
    for Mp in cases.SWEEP_SIZES:
        s = cases.sweep_scenario(Mp)
        inp = make_inputs(s)
        q, bad, row = tolerances(s, inp, SWEEP_QUANT, False)
        print("sweep %4d  tol_disp_2 %.1e | %s" % (Mp, q["tol_disp_2"], "  ".join(row)))
        assert not bad or not write, (Mp, bad)
        if bad:
            print("   FAILS:", "; ".join(bad))
        if Mp == cases.SWEEP_SIZES[0]:
            g.update({k: inp[k] for k in ("obs0", "action", "obs1")})
        # storage (the file's size limit): the float64 twins rounded to fp32 - 6e-8, two orders below the smallest tolerance, which was
        # measured before the rounding - and x_2's twin as the DISPLACEMENT x_2_f64 - x0, taken in float64 (what the test compares)
        q["disp_2_f64"] = (q.pop("x_2_f64").astype(np.float64) - inp["x0"]).astype(np.float32)
        q["phi0_f64"], q["grad_norms_2_f64"] = q["phi0_f64"].astype(np.float32), q["grad_norms_2_f64"].astype(np.float32)
        g.update({"%s_%d" % (k, Mp): v for k, v in q.items()})
    if write:
        np.savez_compressed(os.path.join(mg.OUT, "mpf_cartpole_sweep.npz"), **g)


if __name__ == "__main__":
    dry = "--dry" in sys.argv[1:]  # print the table, assert and write nothing (for choosing a scenario's lr / bw / spread)
    only = set(sys.argv[1:]) - {"--dry"}
    for s in cases.SCENARIOS:
        if not only or s["tag"] in only:
            run(s, write=not dry)
    if not only or "sweep" in only:
        run_sweep(write=not dry)
