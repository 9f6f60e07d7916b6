#!/usr/bin/env python3
"""Golden vectors of the reference's controllers on its SkidSteerRobot with the NAVIGATION cost - a quadratic cost plus
w_obs * obst_map.get_collisions(states[..., 0:2]), the obstacle term of Particle.default_inst_cost / default_term_cost
(particle.py:170-225, obstacle_map.py:64-93), added in that order: quad.sum(-1) + ctrl.sum(-1) + obst.  MultiDISCO.forward, plain and in
the sigma-point form (tests/golden/skid_nav_<tag>.npz), and AMPPI.update_actions (amppi_nav_<tag>.npz), from recorded actions / eps and
parameter rows.

TEST INFRASTRUCTURE.  Run from the repo root:  python tests/golden/make_golden_skid_nav.py [--dry] [tag ...]
Needs the reference (build container only); writes arrays and scalars only.  Scenarios are data in tests/skid_nav_cases.py; the
reference is imported as make_golden_skid.py / make_golden_ut_families.py / make_golden_amppi.py import it.

Tolerances are the project's rule (make_golden_cartpole.tolerances): d = max(fp32 run vs fp32 run with every input moved one ulp, fp32
run vs float64 run), tol = max(1e-5, 2 d), stored; a fixture over 5e-5 is refused.

The cost is DISCONTINUOUS at cell edges, so the inputs must keep the reference itself inside the cap.  Asserted and stored:
  stable cells   the occupancy index of every rollout state is the same in the fp32 run, the one-ulp run and the float64 run;
  edge margin    every state's scaled position p / cell + offset is >= 1e-4 cells from an integer on both axes (`margin`), and the margin
                 is >= 10 x the largest fp32 - float64 difference of that scaled position (`scaled_diff`);
  seed search    the inputs come from the first seed, counted from the scenario's base seed, that meets both (`seed`, `tries` <= 500);
  reach          the share of colliding rollout-steps (`collision_share`) lies in [5 %, 95 %]; the off-map scenario leaves the map on
                 both sides of both axes (`offmap_sides`);
  power          every `costs_off_<variant>` (skid_nav_cases.nav_terms: w0, transpose, round, noterm, shift, free) is >= 10 tol_costs
                 away from the costs, or the fixture is refused;
  restatement    tests/skid_nav_cases.py's float64 restatement reproduces the float64 run to 1e-12.
Maps are stored bit-packed (`map_bits`, `map_shape`) and are skid_nav_cases.make_map's.
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import make_golden as mg  # noqa: E402  (installs the shim, imports the reference)
import make_golden_cartpole as mc  # noqa: E402  (tolerances, moved, pdist_of)
import make_golden_mpf_sizes as ms  # noqa: E402  (_dtype)

import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.distributions as dist  # noqa: E402
from dust.controllers.amppi import AMPPI  # noqa: E402
from dust.models.skid_steer_robot import SkidSteerRobot  # noqa: E402
from dust.utils.obstacle_map import ObstacleMap  # noqa: E402
from dust.utils.utf import MerweScaledUTF  # noqa: E402

sys.path.insert(0, os.path.join(mg.ROOT, "tests"))
import skid_nav_cases as cases  # noqa: E402
from helpers import elemerr  # noqa: E402


def ref_map(s, grid):
    """the reference's ObstacleMap holding `grid` (made inside the run's dtype context: its c_offset is a default-dtype tensor)"""
    om = ObstacleMap(list(s["map_dim"]), s["cell"])
    assert om.map.shape == grid.shape, (om.map.shape, grid.shape)
    om.map = grid.astype(np.float64)
    om.convert_map()
    return om


class NavCost:
    """The cost callable: Particle.default_inst_cost / default_term_cost's expression (particle.py:170-225) with a goal of five entries,
    in the default dtype.  with_actions False: the instantaneous cost ignores its actions (the sigma-point form hands S N pts H states and
    S N H actions, disco.py:306-309; AMPPI hands none, amppi.py:205)."""

    def __init__(self, s, obst_map, with_actions):
        self.goal, self.w_state = torch.tensor(cases.GOAL), torch.tensor(cases.W_STATE)
        self.w_term, self.w_ctrl = torch.tensor(cases.W_TERM), torch.tensor(s["w_ctrl"])
        self.obst_map, self.w_obs, self.with_actions = obst_map, s["w_obs"], with_actions

    def inst(self, states, actions=None, n_pol=1, debug=None):
        obst_cost = self.w_obs * self.obst_map.get_collisions(states[..., 0:2])
        delta = states - self.goal
        state_cost = torch.mul(delta, delta) * self.w_state
        if not self.with_actions:
            return state_cost.sum(-1) + obst_cost
        control_cost = torch.mul(actions, actions) * self.w_ctrl
        return state_cost.sum(-1) + control_cost.sum(-1) + obst_cost

    def term(self, states, n_pol=1, debug=None):
        obst_cost = self.w_obs * self.obst_map.get_collisions(states[..., 0:2])
        delta = states - self.goal
        return (torch.mul(delta, delta) * self.w_term).sum(-1) + obst_cost


def ref_model(s):
    lo, hi = s["bounds"]
    return SkidSteerRobot(delta_t=s["dt"], uncertain_params=s["up"] or None, min_wheel_speed=lo, max_wheel_speed=hi, **s["fixed"])


def transform(s, dt):
    tf = MerweScaledUTF(n=len(s["up"]), alpha=s["alpha"])
    if dt == torch.float64:  # (utf.py:86-87 hard-codes float32 weights: set on the instance, make_golden_ut_families.transform)
        tf._MerweScaledUTF__loc_weights = torch.tensor(cases.weights(len(s["up"]), s["alpha"])[0], dtype=torch.float64)
    return tf


def ref_disco(s, inp, grid, dt=torch.float32):
    """MultiDISCO.forward (kinds "disco" and "ut") -> dict of arrays; states [M, S, N, H + 1, 5]"""
    with ms._dtype(dt):
        t = lambda a: torch.as_tensor(np.asarray(a, np.float32)).to(dt)
        ut = s["kind"] == "ut"
        model, cost = ref_model(s), NavCost(s, ref_map(s, grid), with_actions=not ut)
        tf = transform(s, dt) if ut else None
        ctrl = mg.MultiDISCO(model.observation_space, model.action_space, s["H"], s["N"], s["S"], temperature=cases.TEMPERATURE,
                             ctrl_penalty=s["ctrl_penalty"], a_cov=torch.tensor(cases.a_cov_of(s)).to(torch.get_default_dtype()),
                             inst_cost_fn=cost.inst, term_cost_fn=cost.term, params_sampling=tf if ut else bool(s["up"]), params_samples=s["M"],
                             params_log_space=s["log"])
        ctrl.a_mat = t(inp["a_mat0"]).clone()  # (forward updates it in place)
        ctrl.a_seq = t(inp["a_seq0"]).clone()
        if ut:
            pd = dist.MultivariateNormal(t(inp["dist_mean"]), covariance_matrix=torch.diag(t(inp["dist_std"]) ** 2))
        else:
            pd = mc.pdist_of(s, [inp["params"]] if "params" in inp else None, t)
        with torch.no_grad():
            costs, states, _, omega, _ = ctrl.forward(t(inp["state"]), model, pd, ext_actions=t(inp["ext_actions"]))
        out = dict(costs=mg.npf(costs), omega=mg.npf(omega), a_mat1=mg.npf(ctrl.a_mat), a_mix=mg.npf(ctrl.a_mix))
        if ut:  # [S pts, N, H + 1, 5], rollout (s N + n) pts + k runs sigma point k (disco.py:257-264) -> [pts, S, N, H + 1, 5]
            out["states"] = mg.npf(states.reshape(s["S"], s["N"], tf.pts, s["H"] + 1, -1).permute(2, 0, 1, 3, 4).contiguous())
            out["sigma_points"] = mg.npf(tf.compute_sigma_points(pd.mean, pd.covariance_matrix).T)
            out["loc_weights"] = mg.npf(tf.loc_weights)
        else:
            out["states"] = mg.npf(states).reshape(s["M"], s["S"], s["N"], s["H"] + 1, 5)
        return out


def ref_amppi(s, inp, grid, dt=torch.float32):
    """AMPPI.update_actions, set up as make_golden_amppi.py sets it up -> dict of arrays; states [S pts, H + 1, 5]"""
    with ms._dtype(dt):
        t = lambda a: torch.as_tensor(np.asarray(a, np.float32)).to(dt)
        model, cost = ref_model(s), NavCost(s, ref_map(s, grid), with_actions=False)
        tf = transform(s, dt) if s["mode"] == "ut" else None
        ctrl = AMPPI(model.observation_space, model.action_space, s["H"], s["S"], lambda_=cases.TEMPERATURE,
                     a_cov=torch.as_tensor(cases.a_cov_of(s).astype(np.float32)).to(dt), inst_cost_fn=lambda x: cost.inst(x), term_cost_fn=lambda x: cost.term(x),
                     params_sampling=tf if tf is not None else s["mode"])
        ctrl.a_seq = t(inp["a_seq0"]).clone()
        out = {}
        if "params" in inp:
            model.sample_params = lambda n, r=inp["params"]: model.params_to_dict(t(r)[:n])
        if tf is not None:
            model.params_dist = dist.MultivariateNormal(t(inp["dist_mean"]), covariance_matrix=torch.diag(t(inp["dist_std"]) ** 2))
            model.to_params_dict = model.params_to_dict  # the method amppi.py:182 meant
            out["sigma_points"] = mg.npf(tf.compute_sigma_points(model.params_dist.mean, model.params_dist.covariance_matrix).T)
            out["loc_weights"] = mg.npf(tf.loc_weights)
        with torch.no_grad():
            costs, states, _, omega = ctrl.update_actions(model, t(inp["state"]), t(inp["actions"]))
        out.update(costs=mg.npf(costs), states=mg.npf(states).reshape(-1, s["H"] + 1, 5), omega=mg.npf(omega), a_seq1=mg.npf(ctrl.a_seq))
        return out


KEYS = ("state", "a_mat0", "a_seq0", "ext_actions", "actions", "params", "dist_mean", "dist_std")


def margin_of(s, grid, states32):
    sc = cases.scaled32(states32[..., 0:2], s, grid.shape).astype(np.float64)
    return float(np.abs(sc - np.round(sc)).min())


def search(s, grid):
    """the first seed from the scenario's base whose fp32, one-ulp and float64 runs meet the stable-cell and edge-margin conditions"""
    ref = ref_amppi if s["kind"] == "amppi" else ref_disco
    for k in range(cases.MAX_TRIES):
        seed = s["seed"] + k
        inp = cases.inputs(s, seed)
        r32 = ref(s, inp, grid)
        margin = margin_of(s, grid, r32["states"])
        if margin < cases.MARGIN:
            continue
        rp = ref(s, mc.moved(inp, 9000 + seed, KEYS), grid)
        r64 = ref(s, inp, grid, torch.float64)
        sc32 = cases.scaled32(r32["states"][..., 0:2], s, grid.shape)
        scp = cases.scaled32(rp["states"][..., 0:2], s, grid.shape)
        sc64 = cases.scaled64(r64["states"][..., 0:2], s, grid.shape)
        diff = float(np.abs(sc32.astype(np.float64) - sc64).max())
        stable = np.array_equal(np.floor(sc32), np.floor(scp)) and np.array_equal(np.floor(sc32).astype(np.int64), np.floor(sc64).astype(np.int64))
        if stable and margin >= cases.MARGIN_RATIO * diff and margin_of(s, grid, rp["states"]) > 0:
            return dict(seed=seed, tries=k + 1, margin=margin, scaled_diff=diff, stable_cells=True), inp, (r32, rp, r64)
    raise AssertionError("%s: no seed within %d tries" % (s["tag"], cases.MAX_TRIES))


def run(s, write=True):
    grid = cases.make_map(s)
    amppi = s["kind"] == "amppi"
    cond, inp, (r32, rp, r64) = search(s, grid)
    quant = cases.AMPPI_QUANT if amppi else cases.ROLLOUT_QUANT
    g = dict(kind=s["kind"], S=s["S"], H=s["H"], N=s["N"], M=s["M"], uncertain=",".join(s["up"]), cell=s["cell"], w_obs=s["w_obs"], alpha=s["alpha"],
             map_bits=cases.pack_map(grid), map_shape=np.array(grid.shape), **cond, **inp)
    assert np.array_equal(cases.unpack_map(g), grid)
    bad, row = mc.tolerances((r32, rp, r64), quant, g)
    d = ["%s %.1e" % (q, max(elemerr(rp[q], r32[q]), elemerr(r32[q], r64[q]))) for q in quant]  # the measured error behind each tolerance
    delta = (g.pop("states_f64") - g["states"].astype(np.float64)) * cases.TWIN_SCALE
    g["states_f64_delta32"] = delta.astype(np.float32)
    assert elemerr(cases.twin(g, "states"), r64["states"]) < 1e-12
    if "sigma_points" in r32:
        g["sigma_points"], g["loc_weights"] = r32["sigma_points"], r32["loc_weights"]
        assert np.array_equal(r64["sigma_points"].astype(np.float32), r32["sigma_points"])  # (utf.py:108-118: fp32 in either run)
    if not amppi:
        # MultiDISCO's float64 run keeps the start state in fp32 (disco.py:369): its first step takes the heading's cosine and sine from
        # torch's fp32 routines - recorded, so that a float64 restatement can follow that run without torch (make_golden_skid.py)
        th0 = torch.from_numpy(inp["state"])[2:3]
        g["trig0_f32"] = mg.npf(torch.cat([torch.cos(th0), torch.sin(th0)]))
    # conditions
    occ = cases.occupancy(grid, cases.scaled64(g["states"][..., 0:2], s, grid.shape))
    g["collision_share"] = float(occ.mean())
    if not 0.05 <= g["collision_share"] <= 0.95:
        bad.append("collision share %.3f outside [0.05, 0.95]" % g["collision_share"])
    sc = cases.scaled64(g["states"][..., 0:2], s, grid.shape)
    g["offmap_sides"] = np.array([(sc[..., 0] < 0).mean(), (sc[..., 0] >= grid.shape[0]).mean(), (sc[..., 1] < 0).mean(), (sc[..., 1] >= grid.shape[1]).mean()])
    if "free" in s["offs"] and not g["offmap_sides"].min() > 0.005:
        bad.append("off-map shares %s: every side >= 0.5 %%" % g["offmap_sides"])
    re = (cases.restate_amppi if amppi else cases.restate_disco)(s, g, grid)
    for q in quant:
        e = elemerr(re[q], r64[q])
        assert e < 1e-12, (s["tag"], "the restatement is not the reference's float64 run", q, e)
    power = []
    for v in s["offs"]:
        g["costs_off_" + v] = cases.costs_off(s, g, grid, v)
        p = elemerr(g["costs_off_" + v], g["costs"])
        power.append("%s %.0f" % (v, p / g["tol_costs"]))
        if not p >= 10 * g["tol_costs"]:
            bad.append("power(%s) %.2e < 10 x tol_costs %.1e" % (v, p, g["tol_costs"]))
    if s["S"] > 2:
        g["top_weight"] = float(np.exp(r32["omega"]).max() if amppi else r32["omega"].max())
    print("%-9s seed +%-3d margin %.1e / diff %.1e  hit %2.0f %%  power(tol) %s | %s" % (s["tag"], cond["tries"] - 1, cond["margin"], cond["scaled_diff"],
                                                                                  100 * g["collision_share"], " ".join(power), "  ".join(row)))
    print("          measured d: " + "  ".join(d))
    assert not bad or not write, (s["tag"], bad)
    if bad:
        print("   FAILS:", "; ".join(bad))
    if write:
        path = os.path.join(mg.OUT, cases.fixture_name(s) + ".npz")
        np.savez_compressed(path, **g)
        assert os.path.getsize(path) < 512 * 1024, (s["tag"], os.path.getsize(path))


if __name__ == "__main__":
    dry = "--dry" in sys.argv[1:]  # print the tables, assert and write nothing (for choosing a scenario's inputs)
    only = set(sys.argv[1:]) - {"--dry"}
    for s in cases.ROLLOUTS + cases.AMPPI:
        if not only or s["tag"] in only:
            run(s, write=not dry)
