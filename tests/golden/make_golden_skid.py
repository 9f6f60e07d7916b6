#!/usr/bin/env python3
"""Golden vectors of the reference's controller on its SkidSteerRobot (dust/models/skid_steer_robot.py): MultiDISCO.forward rollouts at
the shapes and options the three round-3 fixtures (make_golden_r3.py) leave out - a partial second block, every column order, log space
with three columns, the scalar-event quirk, asymmetric wheel-speed bounds, a full 2 x 2 a_cov, and ctrl_penalty != 1 (the
control-regularisation term of disco.py:338-346) - as tests/golden/skid_ctrl_<tag>.npz.

TEST INFRASTRUCTURE.  Run from the repo root:  python tests/golden/make_golden_skid.py [--dry] [tag ...]
Needs the reference (build container only); writes arrays and scalars only.

Scenarios are data in tests/skid_cases.py; every recorded array has a leading axis over the scenario's consecutive forward calls.
Tolerances follow make_golden_cartpole.py / make_golden_mpf_sizes.py (read the latter's docstring): per recorded quantity
d = max(elemerr(fp32 run, fp32 run with every input entry moved one ulp), elemerr(fp32 run, float64 run)) - the largest over the calls -
tol = max(1e-5, 2 d), stored next to the quantity's `_f64` twin and asserted <= 5e-5.  The states' twin is stored as `states_f64_delta16`
(cartpole_cases.twin).
Power: the lead quantity (costs; the scalar-event fixture: states) with one thing ignored (the scenario's `off`) as `<lead>_off`, from a
torch restatement of the rollout and of _compute_cost that is first asserted equal to the reference's (states bit for bit, costs to an
ulp); elemerr(off, lead) >= 10 tol is asserted.  What `off` ignores:
  order      the column order of the parameter samples (read as x_icr, wheel_radius)
  exp_ad     the exp of the axial_distance column in log space
  interleave rollout r on params[r % M] (disco.py:177-179): every rollout of block m on params[m] instead
  clamp      the step's clamp of the wheel speeds to the action bounds
  chol_off   the off-diagonal entry of L in actions = a_mat0 + L eps (the costs of the actions a diagonal L makes)
  areg       the whole control-regularisation term;  areg2: that of the second call only
  apre_off   the off-diagonal entry of a_pre = inverse(a_cov) in that term
"""
import math
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import make_golden as mg  # noqa: E402  (installs the shim, imports the reference)
import make_golden_cartpole as mc  # noqa: E402  (the rule's pieces: tolerances, moved, FixedDist)
import make_golden_mpf_sizes as ms  # noqa: E402

import numpy as np  # noqa: E402
import torch  # noqa: E402
from dust.models.skid_steer_robot import SkidSteerRobot  # noqa: E402

sys.path.insert(0, os.path.join(mg.ROOT, "tests"))
import skid_cases as cases  # noqa: E402
from helpers import elemerr  # noqa: E402


class QuadCost:
    """make_golden_r3.py's skid_inst / skid_term in the default dtype"""

    def __init__(self):
        self.goal, self.w_state = torch.tensor(cases.GOAL), torch.tensor(cases.W_STATE)
        self.w_term, self.w_ctrl = torch.tensor(cases.W_TERM), torch.tensor(cases.W_CTRL)

    def inst(self, states, actions=None, n_pol=1, debug=None):
        return (((states - self.goal) ** 2) * self.w_state).sum(-1) + ((actions ** 2) * self.w_ctrl).sum(-1)

    def term(self, states, n_pol=1, debug=None):
        return (((states - self.goal) ** 2) * self.w_term).sum(-1)


def ref_model(s):
    return SkidSteerRobot(delta_t=s["dt"], uncertain_params=s["up"] or None, min_wheel_speed=s["bounds"][0], max_wheel_speed=s["bounds"][1], **s["fixed"])


def controller(s, model, cost):
    return mg.MultiDISCO(model.observation_space, model.action_space, s["H"], s["N"], s["S"], temperature=cases.TEMPERATURE,
                         ctrl_penalty=s["ctrl_penalty"], a_cov=torch.tensor(cases.a_cov_of(s)).to(torch.get_default_dtype()), inst_cost_fn=cost.inst,
                         term_cost_fn=cost.term, params_sampling=bool(s["up"]), params_samples=s["M"], params_log_space=s["log"])


def chol32(s):
    """L of the action covariance in fp32, as the library's configuration forms it: (L00, L10, L11)"""
    if s["a_cov"] is None:
        return np.float32(cases.SIGMA_A), np.float32(0.0), np.float32(cases.SIGMA_A)
    L = torch.linalg.cholesky(torch.tensor(np.asarray(s["a_cov"], np.float32)))
    return np.float32(L[0, 0]), np.float32(L[1, 0]), np.float32(L[1, 1])


def actions_of(s, a_mat0, eps, off=None):
    """a_mat0 + L eps in fp32, in the device's order of operations (skid.hpp, rollout.hpp's tile pass)"""
    l00, l10, l11 = chol32(s)
    e0, e1 = eps[..., 0], eps[..., 1]
    a0 = a_mat0[None, ..., 0] + l00 * e0
    a1 = a_mat0[None, ..., 1] + ((l10 * e0 + l11 * e1) if (l10 != 0 and off != "chol_off") else l11 * e1)
    return np.stack([a0, a1], -1).astype(np.float32)


def rollout_inputs(s):
    rng = np.random.default_rng(s["seed"])
    N, S, H, C = s["N"], s["S"], s["H"], s["calls"]
    a_mat0 = (0.25 * s["act_scale"] * rng.standard_normal((N, H, 2))).astype(np.float32)
    eps = (s["act_scale"] * rng.standard_normal((C, S, N, H, 2))).astype(np.float32)
    a_seq0 = (0.2 * rng.standard_normal((H, 2)) if s["a_seq"] else np.zeros((H, 2))).astype(np.float32)
    inp = dict(state=np.array(cases.STATE0, np.float32), a_mat0=a_mat0, a_seq0=a_seq0, eps=eps,
               ext_actions=np.stack([actions_of(s, a_mat0, e) for e in eps]))
    if s["up"]:
        inp["params"] = mc.draw_params(s, rng, C)
    return inp


def ref_forward(s, inp, dt=torch.float32):
    """the scenario's consecutive forward calls on one controller -> dict of [calls, ...] arrays"""
    with ms._dtype(dt):
        t = lambda a: torch.as_tensor(np.asarray(a, np.float32)).to(dt)
        model, cost = ref_model(s), QuadCost()
        ctrl = controller(s, model, cost)
        ctrl.a_mat = t(inp["a_mat0"]).clone()  # (forward updates it in place)
        ctrl.a_seq = t(inp["a_seq0"]).clone()
        pd = mc.pdist_of(s, inp["params"] if "params" in inp else None, t)
        out = {q: [] for q in cases.ROLLOUT_QUANT}
        for c in range(s["calls"]):
            with torch.no_grad():
                costs, states, actions, omega, _ = ctrl.forward(t(inp["state"]), model, pd, ext_actions=t(inp["ext_actions"][c]))
            for q, v in zip(cases.ROLLOUT_QUANT, (costs, states, omega, ctrl.a_mat, ctrl.a_mix)):
                out[q].append(mg.npf(v))
        return {q: np.stack(v) for q, v in out.items()}


def restated(s, inp, c, a_mat, off=None):
    """MultiDISCO._rollout + _compute_cost over SkidSteerRobot.step in fp32 torch, operation by operation, for call c with the a_mat that call
    sees; `off` ignores one thing.  -> dict(costs [S, N], states [M, S, N, H + 1, 5])"""
    N, S, H, M = s["N"], s["S"], s["H"], s["M"]
    f = torch.from_numpy
    p = dict(s["fixed"])
    if s["up"]:
        raw = f(inp["params"][c])
        if s["log"]:
            ex = raw.exp()
            if off == "exp_ad":
                ex[..., s["up"].index("axial_distance")] = raw[..., s["up"].index("axial_distance")]
            raw = ex
        if s["dist"] == "scalar" and off != "interleave":
            rows = raw.reshape(-1).repeat(1, S * N).reshape(-1, 1)  # disco.py:177-179: rollout r takes params[r % M]
        else:
            rows = raw.reshape(M, -1).repeat(1, S * N).reshape(-1, raw.reshape(M, -1).shape[1])
        up = ("x_icr", "wheel_radius") if off == "order" else s["up"]
        for i, k in enumerate(up):
            p[k] = rows[:, i].reshape(-1, 1)
    x_icr, wheel_radius, axial_distance = (p[k] for k in cases.NAMES3)
    ext = actions_of(s, inp["a_mat0"], inp["eps"][c], off) if off == "chol_off" else inp["ext_actions"][c]
    acts = f(ext).reshape(-1, H, 2).repeat(M, 1, 1)
    lo, hi = (torch.tensor(v, dtype=torch.float) for v in s["bounds"])
    x = f(inp["state"]).expand(M * S * N, -1).clone()
    cost, inst, traj = QuadCost(), [], [x]
    for t in range(H):
        a = acts[:, t]
        inst.append(cost.inst(x, a))
        xx, y, th, _, _ = x.chunk(5, dim=1)
        right, left = a.clone().chunk(2, dim=1)
        if off != "clamp":
            right.clamp_(lo, hi)
            left.clamp_(lo, hi)
        lin = (right + left) * math.pi * wheel_radius
        ang = (right - left) * 2 * math.pi * wheel_radius / axial_distance
        fwd = lin * s["dt"]
        lat = -ang * x_icr * s["dt"]
        nx = xx + fwd * torch.cos(th) - lat * torch.sin(th)
        ny = y + fwd * torch.sin(th) + lat * torch.cos(th)
        x = torch.cat([nx, ny, th + ang * s["dt"], lin.expand_as(xx), ang.expand_as(xx)], dim=1)
        traj.append(x)
    state_cost = (torch.stack(inst, 1).view(M, S, N, H).sum(-1) + cost.term(x).view(M, S, N)).mean(0)
    a_cov = torch.tensor(cases.a_cov_of(s), dtype=torch.float)
    a_pre = torch.inverse(a_cov)
    if off == "apre_off":
        a_pre = torch.diag(torch.diag(a_pre))
    a_reg = 0.0 if (off == "areg" or (off == "areg2" and c == 1)) else cases.TEMPERATURE * (1 - s["ctrl_penalty"])
    e = torch.add(f(ext), -f(inp["a_seq0"]))
    ctrl = (a_reg * torch.tensordot(-e, f(a_mat) @ a_pre, dims=([-2, -1], [-2, -1]))).diagonal(dim1=-2, dim2=-1)
    return dict(costs=mg.npf(state_cost + ctrl), states=mg.npf(torch.stack(traj, 1).view(M, S, N, H + 1, 5)))


def run_rollout(s, write=True):
    inp = rollout_inputs(s)
    r32 = ref_forward(s, inp)
    rp = ref_forward(s, mc.moved(inp, 2000 + s["seed"], ("state", "a_mat0", "a_seq0", "ext_actions", "params")))
    r64 = ref_forward(s, inp, torch.float64)
    lo, hi = s["bounds"]
    g = dict(N=s["N"], S=s["S"], H=s["H"], M=s["M"], calls=s["calls"], uncertain=",".join(s["up"]), off=s["off"],
             clamped_fraction=np.float32(((inp["ext_actions"] < lo) | (inp["ext_actions"] > hi)).mean()), **inp)
    # the reference's float64 run keeps the start state in fp32 (disco.py:369: torch.as_tensor(state, dtype=torch.float)), so its first step
    # takes the heading's cosine and sine from torch's fp32 routines - not always the correctly rounded values; recorded, so that a
    # float64 restatement can follow that run without torch
    th0 = torch.from_numpy(inp["state"]).expand(s["M"] * s["S"] * s["N"], -1).clone().chunk(5, dim=1)[2]
    trig0 = torch.cat([torch.cos(th0), torch.sin(th0)], 1)
    assert bool((trig0 == trig0[0]).all())
    g["trig0_f32"] = mg.npf(trig0[0])
    bad, row = mc.tolerances((r32, rp, r64), cases.ROLLOUT_QUANT, g, per_slice=cases.ROLLOUT_QUANT)
    delta = (g.pop("states_f64") - g["states"].astype(np.float64)) * cases.TWIN_SCALE
    assert np.abs(delta).max() < 6e4, "the difference leaves binary16's range"
    g["states_f64_delta16"] = delta.astype(np.float16)
    assert elemerr(cases.twin(g, "states"), r64["states"]) < 1e-9
    lead = cases.lead_quantity(s)
    a_mats = [inp["a_mat0"]] + list(r32["a_mat1"])  # call c sees the a_mat call c - 1 left
    on = [restated(s, inp, c, a_mats[c]) for c in range(s["calls"])]
    for c in range(s["calls"]):
        assert np.array_equal(on[c]["states"], g["states"][c]), "the restatement is not the reference's rollout"
        assert elemerr(on[c]["costs"], g["costs"][c]) < 2e-7, ("the restatement is not the reference's cost", elemerr(on[c]["costs"], g["costs"][c]))
    g[lead + "_off"] = np.stack([restated(s, inp, c, a_mats[c], s["off"])[lead] for c in range(s["calls"])])
    power = max(elemerr(a, b) for a, b in zip(g[lead + "_off"], g[lead]))
    print("%-12s power(%s) %.2e  beyond the bounds %.0f %%  max|th| %.2f | %s" % (s["tag"], s["off"], power, 100 * float(g["clamped_fraction"]),
                                                                             float(np.abs(g["states"][..., 2]).max()), "  ".join(row)))
    if not power >= 10 * g["tol_" + lead]:
        bad.append("power %.2e < 10 x tol_%s %.1e" % (power, lead, g["tol_" + lead]))
    if s["tag"] == "bounds" and not float(g["clamped_fraction"]) >= 0.2:
        bad.append("clamped fraction %.2f < 0.2" % float(g["clamped_fraction"]))
    assert not bad or not write, (s["tag"], bad)
    if bad:
        print("   FAILS:", "; ".join(bad))
    if write:
        np.savez_compressed(os.path.join(mg.OUT, "skid_ctrl_" + s["tag"] + ".npz"), **g)


if __name__ == "__main__":
    dry = "--dry" in sys.argv[1:]  # print the tables, assert and write nothing (for choosing a scenario's inputs)
    only = set(sys.argv[1:]) - {"--dry"}
    for s in cases.ROLLOUTS:
        if not only or s["tag"] in only:
            run_rollout(s, write=not dry)
