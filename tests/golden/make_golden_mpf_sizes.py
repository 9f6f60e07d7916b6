#!/usr/bin/env python3
"""Golden vectors of the reference's dynamics filter (dust/inference/mpf.py MPF + likelihoods.py GaussianLikelihood) beyond 12
particles, on the branches of the one-step Jacobian no earlier fixture reaches: the `g` column and P = 3, the P = 1 pendulum, the
log-space chain of the pendulum, the speed-clamp mask (all particles / some particles), the Particle's acceleration and speed masks
(per particle, per channel), the obstacle factor, linear-space Particle mass, and 70 ... 1 024 particles (ragged counts included).

TEST INFRASTRUCTURE.  Run from the repo root:  python tests/golden/make_golden_mpf_sizes.py
Needs the reference (build container only); writes tests/golden/mpf_sz_*.npz (arrays and scalars only, allow_pickle=False).

Per fixture (SCENARIOS below), all computed by the reference's own classes:
  inputs      x0, obs0, action, obs1, action2, obs2, bw, lr, obs_std, n_steps, uncertain (comma-joined names), optimizer
  phi0        MPF.phi(bw) on the conditioned likelihood
  x_2, grad_norms_2          a TWO-step optimize() from x0 (the shortest call the multi-workgroup kernels take)
  x_n, grad_norms            the first full optimize(action, obs1, n_steps)
  x_n2, grad_norms2          the second full optimize(action2, obs2, n_steps) of the same filter (optimiser state carried over)
  probe, probe_log_prob      the resulting prior's log_prob at a few probes
  <quantity>_f64             the same quantity from a float64 run of the reference (default dtype float64, inputs = the fp32 inputs
                             widened).  Both models run in float64: the Particle's obstacle map takes double positions.
  phi0_off    phi for the same particles with the branch-defining input moved just off the branch (`off` of the scenario): another
              action / past state, the `g` column detached from the likelihood (g "held fixed": no dg column), the other parameter
              space, or - where the branch is the particle count - the last particle left out (compared on the rows both have).
  tol_<quantity>             see below;  tol_disp_2 = tol_x_2 * rms(x_2) / rms(x_2 - x0) for the two-step DISPLACEMENT comparison.

Tolerances come from the reference alone.  d_q = max( elemerr(fp32 run, fp32 run from x0 with EVERY entry moved one ulp in a seeded
random direction), elemerr(fp32 run, float64 run) ) - the reference's own response to rounding-size disturbance; a kernel that sums in
another order cannot be asked for less.  tol_q = max(1e-5, 2 d_q): the factor 2 because the device's order differs at every step, not
only at the input; 1e-5 is the suite's TOL.  Caps (asserted here): tol_q <= 5e-5, pend_g3_lin <= 3e-4 (its summed norms |a|^2 - 2ab +
|b|^2 are near 100 in fp32; measured at the scenario's bandwidth 0.4: the reference's fp32 phi answers the one-ulp move with 3.5e-5
and is 1.8e-5 from its own float64 phi, so tol_phi0 = 7.0e-5), and tol_disp_2 <= 2e-3 (two steps must move the particles by at least
0.5 % of their rms, or the displacement comparison says nothing).  Power (asserted here): elemerr(phi0_off, phi0) >= 10 tol_phi0 and
>= 10 tol_disp_2 - a fixture that does not move when its branch is ignored is re-chosen, not kept.
Step sizes shrink with the particle count (phi's repulsion term is a sum over particles, not a mean), so the chains are contractions.
"""
import contextlib
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import make_golden as mg  # noqa: E402  (installs the shim, imports the reference)

import numpy as np  # noqa: E402
import torch  # noqa: E402

sys.path.insert(0, os.path.join(mg.ROOT, "tests"))
from helpers import elemerr  # noqa: E402

QUANT = ("phi0", "x_2", "grad_norms_2", "x_n", "grad_norms", "x_n2", "grad_norms2", "probe_log_prob")
CAP, CAP_G3_LIN, CAP_DISP, TOL = 5e-5, 3e-4, 2e-3, 1e-5

PEND_TRUE = dict(g=9.8, length=0.8, mass=1.25)


class _DetachedColumns(mg.GaussianLikelihood):
    """The reference's likelihood with some particle columns cut out of the autograd graph: the one-step prediction sees their values,
    its Jacobian has no such column (what a filter that ignored that column's derivative would compute)."""

    def __init__(self, cols, **kw):
        super().__init__(**kw)
        self._cols = cols

    def sample(self, theta):
        parts = [theta[:, c:c + 1].detach() if c in self._cols else theta[:, c:c + 1] for c in range(theta.shape[1])]
        return super().sample(torch.cat(parts, 1))


@contextlib.contextmanager
def _dtype(dt):
    old = torch.get_default_dtype()
    torch.set_default_dtype(dt)
    try:
        yield
    finally:
        torch.set_default_dtype(old)


def _model(s, true=False):
    if s["kind"] == "pendulum":
        return mg.PendulumModel(**PEND_TRUE) if true else mg.PendulumModel(uncertain_params=tuple(s["up"]))
    return mg.Particle(**mg.PARTICLE_ENV, uncertain_params=["mass"], mass=torch.tensor(3.0 if true else 2.0))


def _step_true(s, obs, act):
    m = _model(s, true=True)
    if s["kind"] == "pendulum":
        return m.step(obs.view(1, -1), act.view(1, 1)).view(-1).detach()
    return m.step(obs, act).detach()


def make_inputs(s):
    """x0 and the observation chain, in fp32, seeded per scenario"""
    torch.manual_seed(s["seed"])
    Mp = s["Mp"]
    if s["kind"] == "pendulum":
        centre = dict(g=9.8, length=1.0, mass=1.0)
        cols = [centre[k] + s["spread"].get(k, 0.15) * torch.randn(Mp) for k in s["up"]]
        x0 = torch.stack(cols, 1).clamp(min=0.3)
    else:
        x0 = (2.0 + s["spread"]["mass"] * torch.randn(Mp, 1)).clamp(min=0.5)
    if s["log"]:
        x0 = x0.log()
    obs0, action = torch.tensor(s["obs0"]), torch.tensor(s["action"])
    # (obs1 given: an observation that does not come from the true model - the filter takes any - so that the second call starts elsewhere)
    obs1 = _step_true(s, obs0, action) if s["obs1"] is None else torch.tensor(s["obs1"])
    action2 = action * 0.5
    obs2 = _step_true(s, obs1, action2)
    return dict(x0=mg.npf(x0), obs0=mg.npf(obs0), action=mg.npf(action).reshape(-1), obs1=mg.npf(obs1), action2=mg.npf(action2).reshape(-1),
                obs2=mg.npf(obs2))


def _filter(s, x0, obs0, log=None, detach=()):
    model = _model(s)
    log = s["log"] if log is None else log
    kw = dict(initial_obs=obs0, obs_std=s["obs_std"], model=model, log_space=log)
    lik = _DetachedColumns(detach, **kw) if detach else mg.GaussianLikelihood(**kw)
    if s["opt"] == "Adam":  # the class default of SVGD (svgd.py:115)
        f = mg.MPF(init_particles=x0.clone(), likelihood=lik, lr=s["lr"], bw=s["bw"], bw_scale=1.0)
        assert isinstance(f.optimizer, torch.optim.Adam)
    else:
        f = mg.MPF(init_particles=x0.clone(), likelihood=lik, optimizer_class=torch.optim.SGD, lr=s["lr"], bw=s["bw"], bw_scale=1.0)
    return f, lik


def ref_phi(s, inp, dt=torch.float32, x0=None, **off):
    """one MPF.phi(bw) of the reference; off: obs0 / action overrides, log, detach"""
    with _dtype(dt):
        t = lambda a: torch.as_tensor(np.asarray(a, np.float32)).to(dt)
        x = t(inp["x0"] if x0 is None else x0)
        f, lik = _filter(s, x, t(off.get("obs0", inp["obs0"])), log=off.get("log"), detach=off.get("detach", ()))
        a = t(off.get("action", inp["action"]))
        lik.condition(a if s["kind"] == "particle" else a.reshape(()), t(inp["obs1"]))
        return f.phi(s["bw"]).detach().cpu().numpy().copy()


def ref_run(s, inp, dt=torch.float32, x0=None):
    """every recorded quantity of one scenario from the reference, in dtype dt"""
    out = dict(phi0=ref_phi(s, inp, dt, x0))
    with _dtype(dt):
        t = lambda a: torch.as_tensor(np.asarray(a, np.float32)).to(dt)
        act = lambda a: t(a) if s["kind"] == "particle" else t(a).reshape(())
        x = t(inp["x0"] if x0 is None else x0)
        f, _ = _filter(s, x, t(inp["obs0"]))
        gn, _ = f.optimize(act(inp["action"]), t(inp["obs1"]), bw=s["bw"], n_steps=2)
        out.update(x_2=mg.npf(f.x), grad_norms_2=mg.npf(gn))
        f, _ = _filter(s, x, t(inp["obs0"]))
        gn, _ = f.optimize(act(inp["action"]), t(inp["obs1"]), bw=s["bw"], n_steps=s["n"])
        out.update(x_n=mg.npf(f.x), grad_norms=mg.npf(gn))
        gn, _ = f.optimize(act(inp["action2"]), t(inp["obs2"]), bw=s["bw"], n_steps=s["n"])
        out.update(x_n2=mg.npf(f.x), grad_norms2=mg.npf(gn))
        lo, hi = float(inp["x0"].min()) - 0.5, float(inp["x0"].max()) + 0.5
        probe = torch.linspace(lo, hi, 7).view(-1, 1).expand(-1, x.shape[1]).contiguous().to(dt)
        out.update(probe=mg.npf(probe).astype(np.float32), probe_log_prob=mg.npf(f.prior.log_prob(probe)))
    return out


def one_ulp(x, seed):
    rng = np.random.default_rng(seed)
    d = np.where(rng.random(x.shape) < 0.5, -np.inf, np.inf).astype(np.float32)
    return np.nextafter(x, d).astype(np.float32)


def run(s, write=True):
    tag = s["tag"]
    inp = make_inputs(s)
    r32 = ref_run(s, inp)
    rp = ref_run(s, inp, x0=one_ulp(inp["x0"], 1000 + s["seed"]))
    try:
        r64 = ref_run(s, inp, torch.float64)
    except Exception as e:  # noqa: BLE001 - a model that refuses double tensors: the fixture goes without the _f64 keys
        print("  (%s: no float64 run: %s)" % (tag, e))
        r64 = None
    g = dict(Mp=s["Mp"], P=inp["x0"].shape[1], n_steps=s["n"], log_space=int(s["log"]), bw=s["bw"], lr=s["lr"], obs_std=s["obs_std"],
             model_kind=s["kind"], optimizer=s["opt"], uncertain=",".join(s["up"]), **inp)
    cap = CAP_G3_LIN if tag == "pend_g3_lin" else CAP
    row, bad = [], []
    for q in QUANT:
        g[q] = r32[q]
        d = dp = elemerr(rp[q], r32[q])
        if r64 is not None:
            g[q + "_f64"] = r64[q]
            d = max(d, elemerr(r32[q], r64[q]))
        g["tol_" + q] = max(TOL, 2.0 * d)
        row.append("%s %.1e%s" % (q, g["tol_" + q], "" if g["tol_" + q] == TOL else " (ulp)" if d == dp else " (f64)"))
        if g["tol_" + q] > cap:
            bad.append("%s %.1e > cap %.0e" % (q, g["tol_" + q], cap))
    g["probe"] = r32["probe"]
    rms = lambda a: float(np.sqrt(np.mean(np.asarray(a, np.float64) ** 2)))
    g["tol_disp_2"] = g["tol_x_2"] * rms(r32["x_2"]) / rms(r32["x_2"].astype(np.float64) - inp["x0"])
    if g["tol_disp_2"] > CAP_DISP:
        bad.append("tol_disp_2 %.1e > cap %.0e" % (g["tol_disp_2"], CAP_DISP))
    off = dict(s["off"])
    if off.pop("drop_last", False):
        phi_off = ref_phi(s, inp, x0=inp["x0"][:-1])
        power = elemerr(phi_off, r32["phi0"][:-1])
    else:
        phi_off = ref_phi(s, inp, **off)
        power = elemerr(phi_off, r32["phi0"])
    g["phi0_off"] = phi_off
    moved = float(np.abs(r32["x_n"].astype(np.float64) - inp["x0"]).max())
    print("%-15s Mp %4d  power %.2e  tol_disp_2 %.1e  max move %.3f | %s" % (tag, s["Mp"], power, g["tol_disp_2"], moved, "  ".join(row)))
    if not (power >= 10 * g["tol_phi0"] and power >= 10 * g["tol_disp_2"]):
        bad.append("power %.2e < 10 x (tol_phi0 %.1e, tol_disp_2 %.1e)" % (power, g["tol_phi0"], g["tol_disp_2"]))
    assert not bad or not write, (tag, bad, "change lr / bw / spread of the scenario, not the caps")
    if bad:
        print("   FAILS:", "; ".join(bad))
    assert all(np.isfinite(v).all() for v in g.values() if isinstance(v, np.ndarray))
    if write:
        np.savez_compressed(os.path.join(mg.OUT, "mpf_sz_" + tag + ".npz"), **g)
    return g


def S(tag, kind, up, Mp, log, bw, lr, n, off, obs0=None, action=None, spread=None, opt="SGD", seed=0, obs_std=None, obs1=None):
    if obs_std is None:  # (the Particle's one-step Jacobian is small - dt a / m^2: a tighter observation keeps the likelihood visible in phi)
        obs_std = 0.1 if kind == "pendulum" else 0.02
    if obs0 is None:
        obs0 = [3.0, 0.0] if kind == "pendulum" else [-9.0, -9.0, 0.5, -0.25]
    if action is None:
        action = 1.3 if kind == "pendulum" else [10.0, -14.0]
    return dict(tag=tag, kind=kind, up=up, Mp=Mp, log=log, bw=bw, lr=lr, n=n, off=off, obs0=obs0, action=action, spread=spread or {},
                opt=opt, seed=seed, obs_std=obs_std, obs1=obs1)


GLM, LM, PM = ("g", "length", "mass"), ("length", "mass"), ("mass",)
# What each scenario's `off` (9th argument -> phi0_off, the `power` column) means - read it before re-choosing lr / bw / spread:
#   pend_g3_lin, pend_g3_log   detach=(0,): the g column cut out of the likelihood's graph = a Jacobian without its dg column
#   pend_m1_log                log=False: the particles read as linear masses.  This moves the prediction as well as the chain factor, so
#                              its power (45) only says that the space matters; the chain factor itself is held by the 1e-5 on phi0
#   pend_lm_600, pend_lm_1024, part_log_1021   drop_last: the last particle left out - power against a key loop that stops short (the
#                              ragged last row), NOT against a Jacobian branch; it is of order 1 / (neighbours of the last particle)
#   pend_sat, pend_sat_split   past speed 6.0: no particle reaches max_speed, the mask is all ones
#   part_lin                   log=True: the linear masses read as log masses (as pend_m1_log: space, not one factor)
#   part_acc_sat, part_acc_split   a smaller action: no particle reaches max_acc, live_a is all ones
#   part_vel_sat               past v_x 4.0: no particle reaches max_speed, live_v is all ones
#   part_in_obst               past position (-8, -8), outside the obstacle: om = 1
#   pend_adam_300, part_adam_130   half the action: these two are about Adam's state across calls; phi0 has no branch of its own there
# A clamp fixture needs a residual on the clamped channel: a particle whose prediction sits ON the clamp while the observation sits there
# too has y - f = 0, and J^T (y - f) is then zero whatever the mask does.  So the observed speed stays off the clamp: the pendulum's obs1
# is given (7.6 / 7.8 < max_speed 8), part_acc_sat's true mass 3 leaves 27 / 3 = 9 < max_acc 10 while the particles (mass ~2) clamp, and
# part_vel_sat's true next v_x is 4.99 < max_speed 5 while the particles' is clamped.  (tests/test_oracle_golden.py asserts this.)
SCENARIOS = [
    S("pend_g3_lin", "pendulum", GLM, 130, False, 0.4, 0.03 / 130, 10, dict(detach=(0,)), obs0=[1.5, 0.5], spread=dict(g=0.3), obs_std=0.03, seed=101),
    S("pend_g3_log", "pendulum", GLM, 300, True, 0.35, 0.02 / 300, 10, dict(detach=(0,)), obs0=[1.5, 0.5], spread=dict(g=0.3), obs_std=0.03, seed=102),
    S("pend_m1_log", "pendulum", PM, 70, True, 0.3, 0.02 / 70, 20, dict(log=False), seed=103),
    S("pend_lm_600", "pendulum", LM, 600, False, 0.15, 0.016 / 600, 8, dict(drop_last=True), seed=104),
    S("pend_lm_1024", "pendulum", LM, 1024, False, 0.2, 0.035 / 1024, 6, dict(drop_last=True), seed=105),
    S("pend_sat", "pendulum", LM, 130, False, 0.15, 0.012 / 130, 8, dict(obs0=[1.5, 6.0]), obs0=[1.5, 7.9], action=2.0, obs1=[1.88, 7.6], seed=106),
    S("pend_sat_split", "pendulum", LM, 130, False, 0.15, 0.012 / 130, 8, dict(obs0=[1.5, 6.0]), obs0=[1.5, 6.95], action=2.0, obs1=[1.89, 7.8], seed=107),
    S("part_lin", "particle", PM, 130, False, 0.5, 0.05 / 130, 10, dict(log=True), spread=dict(mass=0.1), seed=108),
    S("part_acc_sat", "particle", PM, 130, True, 0.5, 0.1 / 130, 10, dict(action=[10.0, -14.0]), action=[27.0, -14.0], spread=dict(mass=0.1), seed=109),
    S("part_vel_sat", "particle", PM, 130, True, 0.5, 0.1 / 130, 10, dict(obs0=[-9.0, -9.0, 4.0, -0.25]), obs0=[-9.0, -9.0, 4.95, -0.25],
      action=[8.0, -14.0], spread=dict(mass=0.1), seed=110),
    S("part_acc_split", "particle", PM, 300, False, 0.5, 0.05 / 300, 10, dict(action=[14.0, -14.0]), action=[19.0, -21.0], spread=dict(mass=0.15), seed=111),
    S("part_in_obst", "particle", PM, 130, True, 0.5, 0.1 / 130, 10, dict(obs0=[-8.0, -8.0, 0.5, -0.25]), obs0=[-6.0, -6.0, 0.5, -0.25],
      obs1=[-8.0, -8.0, 0.6, -0.3], spread=dict(mass=0.1), seed=112),
    S("part_log_1021", "particle", PM, 1021, True, 0.1, 1e-5, 10, dict(drop_last=True), spread=dict(mass=0.4), seed=113),
    S("pend_adam_300", "pendulum", LM, 300, False, 0.15, 3e-3, 10, dict(action=0.65), opt="Adam", obs_std=0.03, seed=114),
    S("part_adam_130", "particle", PM, 130, True, 0.5, 3e-3, 10, dict(action=[5.0, -7.0]), opt="Adam", spread=dict(mass=0.1), seed=115),
]
NAMES = [s["tag"] for s in SCENARIOS]


if __name__ == "__main__":
    dry = "--dry" in sys.argv[1:]  # print the table, assert and write nothing (for choosing a scenario's lr / bw / spread)
    only = set(sys.argv[1:]) - {"--dry"}
    for s in SCENARIOS:
        if not only or s["tag"] in only:
            run(s, write=not dry)
