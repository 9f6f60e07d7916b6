"""The skid-steer controller fixtures (tests/golden/skid_ctrl_<tag>.npz, made by tests/golden/make_golden_skid.py from the scenarios of
tests/skid_cases.py) without a GPU: every fixture keeps the caps and the power condition its generator asserted, and a float64 numpy
restatement of MultiDISCO.forward on SkidSteerRobot - the rollouts, the control-regularisation term through the full a_pre, the weights
and the a_mat update - reproduces the reference's own float64 run of every fixture to 1e-12.
"""
import numpy as np
import pytest

import skid_cases as cases
from helpers import elemerr

TOL, CAP = 1e-5, 5e-5  # make_golden_mpf_sizes.py


def rollout_f64(s, g, off=None):
    """MultiDISCO.forward on SkidSteerRobot with the quadratic cost, restated in float64 numpy from a fixture's fp32 inputs: the rollouts
    (skid_steer_robot.py:73-122 under disco.py:139-209), the costs with the control-regularisation term (disco.py:294-346) through the full
    a_pre, the weights and the a_mat update (disco.py:380-393), call after call.  -> dict of the cases.ROLLOUT_QUANT arrays [calls, ...]"""
    N, S, H, M = s["N"], s["S"], s["H"], s["M"]
    f = lambda a: np.asarray(a, np.float64)
    goal, w_state, w_term, w_ctrl = f(cases.GOAL), f(cases.W_STATE), f(cases.W_TERM), f(cases.W_CTRL)
    a_pre = np.linalg.inv(cases.a_cov_of(s))
    a_reg = cases.TEMPERATURE * (1 - s["ctrl_penalty"])
    a_mat, a_seq = f(g["a_mat0"]).copy(), f(g["a_seq0"])
    out = {q: [] for q in cases.ROLLOUT_QUANT}
    for c in range(s["calls"]):
        p = {k: np.full((M * S * N, 1), v) for k, v in s["fixed"].items()}
        if s["up"]:
            raw = f(g["params"][c])
            raw = np.exp(raw) if s["log"] else raw
            if s["dist"] == "scalar":
                rows = np.tile(raw.reshape(1, -1), (1, S * N)).reshape(-1, 1)  # disco.py:177-179: rollout r takes params[r % M]
            else:
                rows = np.tile(raw.reshape(M, -1), (1, S * N)).reshape(-1, raw.reshape(M, -1).shape[1])
            for i, k in enumerate(s["up"]):
                p[k] = rows[:, i:i + 1]
        acts = f(g["ext_actions"][c])
        rep = np.tile(acts.reshape(-1, H, 2), (M, 1, 1))
        x = np.tile(f(g["state"]).reshape(1, 5), (M * S * N, 1))
        tot, traj = np.zeros(M * S * N), [x]
        lo, hi = (float(np.float32(v)) for v in s["bounds"])  # (the action space holds its bounds in fp32: skid_steer_robot.py:51-53)
        for t in range(H):
            a = rep[:, t]
            tot = tot + (((x - goal) ** 2) * w_state).sum(-1) + ((a ** 2) * w_ctrl).sum(-1)
            r, l = np.clip(a[:, 0:1], lo, hi), np.clip(a[:, 1:2], lo, hi)
            lin = (r + l) * np.pi * p["wheel_radius"]
            ang = (r - l) * 2 * np.pi * p["wheel_radius"] / p["axial_distance"]
            fwd, lat = lin * s["dt"], -ang * p["x_icr"] * s["dt"]
            th = x[:, 2:3]
            cs, sn = np.cos(th), np.sin(th)
            if t == 0:  # the reference's float64 run keeps the start state in fp32 (disco.py:369): its first step takes the heading's cosine
                cs, sn = (float(v) for v in g["trig0_f32"])  # and sine from torch's fp32 routines - recorded in the fixture
            x = np.concatenate([x[:, 0:1] + fwd * cs - lat * sn, x[:, 1:2] + fwd * sn + lat * cs, th + ang * s["dt"],
                                lin, ang], 1)
            traj.append(x)
        costs = (tot + (((x - goal) ** 2) * w_term).sum(-1)).reshape(M, S, N).mean(0)
        eps = acts - a_seq
        if not (off == "areg" or (off == "areg2" and c == 1)):
            pre = a_pre * np.eye(2) if off == "apre_off" else a_pre
            costs = costs + a_reg * np.einsum("snhd,nhd->sn", -eps, a_mat @ pre)
        log_costs = -1 * (costs - costs.min()) / cases.TEMPERATURE
        mx = log_costs.max(0)
        eta = mx + np.log(np.exp(log_costs - mx).sum(0))
        omega = np.exp(log_costs - eta)
        a_mat = a_mat + np.einsum("sn,snhd->nhd", omega, eps)
        out["costs"].append(costs)
        out["states"].append(np.stack(traj, 1).reshape(M, S, N, H + 1, 5))
        out["omega"].append(omega)
        out["a_mat1"].append(a_mat.copy())
        out["a_mix"].append(np.exp(eta - (eta.max() + np.log(np.exp(eta - eta.max()).sum()))))
    return {q: np.stack(v) for q, v in out.items()}


@pytest.mark.parametrize("name", cases.ROLLOUT_NAMES)
def test_fixture_caps_and_power(golden, name):
    """1e-5 <= tol <= 5e-5 and 2 elemerr(q, q_f64) <= tol per quantity and call; the lead quantity is >= 10 tol from its `_off` variant; the
    shapes are the scenario's"""
    g, s = golden("skid_ctrl_" + name), cases.ROLLOUT_BY_TAG[name]
    C, N, S, H, M = s["calls"], s["N"], s["S"], s["H"], s["M"]
    for q in cases.ROLLOUT_QUANT:
        tol = float(g["tol_" + q])
        assert TOL <= tol <= CAP, (q, tol)
        t64 = cases.twin(g, q)
        assert t64.dtype == np.float64 and t64.shape == g[q].shape and g[q].dtype == np.float32
        d = max(elemerr(a, b) for a, b in zip(g[q], t64))
        slack = 0.0 if q + "_f64" in g else 1e-9  # (a twin stored as a binary16 difference: cartpole_cases.twin)
        assert 2.0 * d <= tol * (1 + 1e-12) + slack, (q, d, tol)
    lead = cases.lead_quantity(s)
    power = max(elemerr(a, b) for a, b in zip(g[lead + "_off"], g[lead]))
    assert power >= 10 * float(g["tol_" + lead]), power
    assert g["costs"].shape == (C, S, N) and g["states"].shape == (C, M, S, N, H + 1, 5) and g["ext_actions"].shape == g["eps"].shape == (C, S, N, H, 2)
    assert bool(np.any(g["a_seq0"] != 0)) == s["a_seq"]
    if s["up"]:
        assert g["params"].shape == (C, M, len(s["up"])) and str(g["uncertain"]) == ",".join(s["up"])
    if name == "ragged":
        assert N * S == 333 and (H * 2) % 8 != 0
    if name == "scalar":
        assert (N * S) % M != 0
    if name == "areg_two":  # the second call's a_mat is the one the first call moved
        assert C == 2 and elemerr(g["a_mat1"][0], g["a_mat0"]) > 1e-2 and elemerr(g["costs_off"][0], g["costs"][0]) < 2e-7


def test_bounds_fixture_clamps_a_fifth(golden):
    g, s = golden("skid_ctrl_bounds"), cases.ROLLOUT_BY_TAG["bounds"]
    lo, hi = s["bounds"]
    frac = float(((g["ext_actions"] < lo) | (g["ext_actions"] > hi)).mean())
    assert abs(frac - float(g["clamped_fraction"])) < 1e-6 and frac >= 0.2
    assert float((g["ext_actions"] < lo).mean()) > 0.05 and float((g["ext_actions"] > hi).mean()) > 0.05  # (either bound)


@pytest.mark.parametrize("name", cases.ROLLOUT_NAMES)
def test_float64_restatement_matches_the_twins(golden, name):
    """rollout_f64 against every `_f64` twin to 1e-12.  The states' twin is stored as a binary16 difference: an entry is held to what that
    storage keeps - 2^-11 of the stored difference (binary16's 11-bit significand) and half its smallest step, 2^-25, both over
    TWIN_SCALE - plus the same 1e-12; the costs, which are sums over those states, are held to 1e-12 outright."""
    g, s = golden("skid_ctrl_" + name), cases.ROLLOUT_BY_TAG[name]
    r = rollout_f64(s, g)
    for q in ("costs", "omega", "a_mat1", "a_mix"):
        assert g[q + "_f64"].dtype == np.float64
        e = elemerr(r[q], g[q + "_f64"])
        assert e < 1e-12, (q, e)
    d16 = np.abs(g["states_f64_delta16"].astype(np.float64))
    t64 = cases.twin(g, "states")
    bound = (2.0 ** -11 * d16 + 2.0 ** -25) / cases.TWIN_SCALE + 1e-12 * (np.abs(t64) + np.sqrt(np.mean(t64 ** 2)))
    assert np.all(np.abs(r["states"] - t64) <= bound), float((np.abs(r["states"] - t64) / bound).max())
    # with its one thing ignored the restatement is the fixture's `_off` variant (fp32 there: to the tolerance), where it can ignore it
    lead = cases.lead_quantity(s)
    if s["off"] in ("areg", "areg2", "apre_off"):
        off = rollout_f64(s, g, s["off"])[lead]
        assert max(elemerr(a, b) for a, b in zip(g[lead + "_off"], off)) < float(g["tol_" + lead])
