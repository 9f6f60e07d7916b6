#!/usr/bin/env python3
"""Golden vectors of the reference's AMPPI controller (dust/controllers/amppi.py): `update_actions` on its PendulumModel, CartPoleModel,
SkidSteerRobot and Particle in the four parameter modes ("none" / "single" / "extended" / MerweScaledUTF), from recorded actions and
parameter rows (amppi_<tag>.npz), and a closed loop of update_actions / roll / plant step (amppi_pend_loop.npz).

TEST INFRASTRUCTURE.  Run from the repo root:  python tests/golden/make_golden_amppi.py [--dry] [tag ...]
Needs the reference (build container only); writes arrays and scalars only.  Scenarios are data in tests/amppi_cases.py.

The reference is imported as make_golden_ut_families.py imports it: through the shim, the cart-pole's name-mangled attribute set on the
instance, the float64 sigma weights set on the instance.  Two more things are set ON THE INSTANCE (no reference text is changed):
`model.to_params_dict = model.params_to_dict` - amppi.py:182 calls a method the reference never defines - and `model.sample_params`, a
function that hands out the recorded rows in place of draws.  `init_actions` cannot be a tensor there (`if not init_actions`, base.py:34):
the start sequence is assigned to `a_seq` after construction.

Tolerances follow make_golden_cartpole.tolerances: every fixture runs in fp32, in fp32 with every input moved one ulp, and in float64;
d = max of the two distances, tol = max(1e-5, 2 d), stored; a fixture over 5e-5 is refused.  Asserted besides (conditions, not
measurements): for S > 2 the largest weight e^omega is <= 0.5; the update moves a_seq by >= 100 tol_a_seq1; the float64 restatement
of tests/amppi_cases.py reproduces the float64 run to 1e-12; each power variant (`costs_disco`: the instantaneous cost on t = 0 .. H - 1;
`costs_noctrl`: no lambda term; `costs_single`: row 0 for every trajectory; `costs_mean`: the plain mean over the sigma points;
`a_seq1_noclamp`) lies >= 10 tol from the true quantity.  The closed loop carries `costs_disco`, `costs_noctrl` and `costs_single` per tick.
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
from dust.controllers.amppi import AMPPI  # noqa: E402
from dust.models.skid_steer_robot import SkidSteerRobot  # noqa: E402
from dust.utils.utf import MerweScaledUTF  # noqa: E402

sys.path.insert(0, os.path.join(mg.ROOT, "tests"))
import amppi_cases as cases  # noqa: E402
import cartpole_cases as cpc  # noqa: E402
from helpers import elemerr  # noqa: E402

CAP, TOL = ms.CAP, ms.TOL


class Cost:
    """inst(x) = sum w_state (x - goal)^2, term(x) = sum w_term (x - goal)^2, in the default dtype"""

    def __init__(self, f):
        self.goal, self.w_state, self.w_term = torch.tensor(f["goal"]), torch.tensor(f["w_state"]), torch.tensor(f["w_term"])

    def inst(self, states):
        return (((states - self.goal) ** 2) * self.w_state).sum(-1)

    def term(self, states):
        return (((states - self.goal) ** 2) * self.w_term).sum(-1)


def ref_model(s):
    """-> (model, inst_cost_fn, term_cost_fn) of the reference"""
    f = cases.FAMILY[s["family"]]
    up = tuple(s["up"]) or None
    if s["family"] == "pendulum":
        return mg.PendulumModel(uncertain_params=up, **f["defaults"]), mg.pend_inst_cost, mg.pend_term_cost
    if s["family"] == "cartpole":
        c = Cost(f)
        return gc.ref_model(f["defaults"], s["up"], dt=f["dt"]), c.inst, c.term
    if s["family"] == "skid":
        c = Cost(f)
        m = SkidSteerRobot(delta_t=f["dt"], min_wheel_speed=torch.tensor(f["lo"], dtype=torch.float32),
                           max_wheel_speed=torch.tensor(f["hi"], dtype=torch.float32), uncertain_params=up, **f["defaults"])
        return m, c.inst, c.term
    assert set(cases.PART_ENV) == set(mg.PARTICLE_ENV)  # (the demo's environment with this scenario's start state and cost weights)
    m = mg.Particle(**cases.PART_ENV, uncertain_params=list(s["up"]) or None, mass=f["defaults"]["mass"])
    assert (m.target.numpy() == np.asarray(f["target"])).all() and m.dt == f["dt"]
    return m, m.default_inst_cost, m.default_term_cost


def transform(n, dt):
    tf = MerweScaledUTF(n=n, alpha=cases.UT_ALPHA)
    if dt == torch.float64:
        tf._MerweScaledUTF__loc_weights = torch.tensor(cases.weights(n)[0], dtype=torch.float64)
    return tf


def controller(s, dt):
    """-> (ctrl, model, tf) with the recorded-row and alias functions in place"""
    f = cases.FAMILY[s["family"]]
    model, inst, term = ref_model(s)
    tf = transform(len(s["up"]), dt) if s["mode"] == "ut" else None
    ctrl = AMPPI(model.observation_space, model.action_space, s["H"], s["S"], lambda_=f["lam"],
                 a_cov=torch.as_tensor(cases.a_cov_of(s)).to(dt), inst_cost_fn=inst, term_cost_fn=term,
                 params_sampling=tf if tf is not None else s["mode"])
    return ctrl, model, tf


def feed(model, rows, t):
    """model.sample_params hands out the recorded rows"""
    model.sample_params = lambda n, r=rows: model.params_to_dict(t(r)[:n])


def ref_update(s, inp, dt=torch.float32):
    with ms._dtype(dt):
        t = lambda a: torch.as_tensor(np.asarray(a, np.float32)).to(dt)
        ctrl, model, tf = controller(s, dt)
        ctrl.a_seq = t(inp["a_seq0"]).clone()
        out = {}
        if "params" in inp:
            feed(model, inp["params"], t)
        if tf is not None:
            model.params_dist = dist.MultivariateNormal(t(inp["dist_mean"]), covariance_matrix=torch.diag(t(inp["dist_std"]) ** 2))
            model.to_params_dict = model.params_to_dict  # the method amppi.py:182 meant
            out["sigma_points"] = mg.npf(tf.compute_sigma_points(model.params_dist.mean, model.params_dist.covariance_matrix).T)
            out["loc_weights"] = mg.npf(tf.loc_weights)
        with torch.no_grad():
            costs, states, acts, omega = ctrl.update_actions(model, t(inp["state"]), t(inp["actions"]))
        out.update(costs=mg.npf(costs), states=mg.npf(states), omega=mg.npf(omega), a_seq1=mg.npf(ctrl.a_seq))
        if s["family"] == "particle":
            out["grid"] = np.asarray(model.obst_map.map, np.float32)
            xy = states[..., :2].reshape(-1, 2)
            out["collisions"] = float(model.obst_map.get_collisions(xy).mean())
    return out


def grid_of(s):
    if s["family"] != "particle":
        return None
    from oracle import grid_4x4_map

    return grid_4x4_map()


def run(s, write=True):
    inp = cases.inputs(s)
    keys = ("state", "a_seq0", "actions", "params", "dist_mean", "dist_std")
    r32 = ref_update(s, inp)
    rp = ref_update(s, gc.moved(inp, 5000 + s["seed"], keys))
    r64 = ref_update(s, inp, torch.float64)
    f = cases.FAMILY[s["family"]]
    g = dict(S=s["S"], H=s["H"], P=len(s["up"]), mode=s["mode"], family=s["family"], uncertain=",".join(s["up"]), lam=f["lam"], **inp)
    quant = cases.QUANT + (("states",) if s["states"] else ())
    bad, row = gc.tolerances((r32, rp, r64), quant, g)
    if s["states"]:
        delta = (g.pop("states_f64") - g["states"].astype(np.float64)) * cpc.TWIN_SCALE
        g["states_f64_delta32"] = delta.astype(np.float32)
        assert elemerr(cases.twin(g, "states"), r64["states"]) < 1e-13
    grid = grid_of(s)
    if grid is not None:
        assert np.array_equal(grid, r32["grid"]), "oracle.grid_4x4_map is not the reference's map"
    sp = None
    if s["mode"] == "ut":
        g["sigma_points"], g["loc_weights"] = r32["sigma_points"], r32["loc_weights"]
        sp = r32["sigma_points"]
        assert np.array_equal(r64["sigma_points"].astype(np.float32), sp)  # (utf.py:108-118: fp32 in either run)
    # the restatement is the reference's float64 run
    re = cases.restate(s, inp, grid=grid, sigma_points=sp)
    for q in ("costs", "omega", "a_seq1", "states"):
        e = elemerr(re[q], r64[q])
        assert e < 1e-12, (s["tag"], q, e)
    # conditions
    top = float(np.exp(r32["omega"]).max())
    if s["S"] > 2 and not top <= 0.5:
        bad.append("top weight %.3f > 0.5" % top)
    move = elemerr(g["a_seq1"], inp["a_seq0"])
    if not move >= 100 * g["tol_a_seq1"]:
        bad.append("a_seq moves %.2e < 100 x tol %.1e" % (move, g["tol_a_seq1"]))
    # power variants
    variants = ["disco", "noctrl"] + (["single"] if s["mode"] == "extended" else []) + (["mean"] if s["mode"] == "ut" else [])
    power = []
    for v in variants:
        g["costs_" + v] = cases.restate(s, inp, variant=v, grid=grid, sigma_points=sp)["costs"].astype(np.float32)
        power.append((v, elemerr(g["costs_" + v], g["costs"]), g["tol_costs"]))
    if s.get("a_seq0") == "edge":
        g["a_seq1_noclamp"] = cases.restate(s, inp, variant="noclamp", grid=grid, sigma_points=sp)["a_seq1"].astype(np.float32)
        power.append(("noclamp", elemerr(g["a_seq1_noclamp"], g["a_seq1"]), g["tol_a_seq1"]))
    for v, p, tol in power:
        if not p >= 10 * tol:
            bad.append("power(%s) %.2e < 10 x tol %.1e" % (v, p, tol))
    extra = "  crashed %.0f %%" % (100 * r32["collisions"]) if "collisions" in r32 else ""
    print("%-15s top %.3f  move %.1e  power %s%s | %s" % (s["tag"], top, move, " ".join("%s %.1e" % (v, p) for v, p, _ in power), extra, "  ".join(row)))
    assert not bad or not write, (s["tag"], bad)
    if bad:
        print("   FAILS:", "; ".join(bad))
    if write:
        np.savez_compressed(os.path.join(mg.OUT, "amppi_" + s["tag"] + ".npz"), **g)
    return g


# ---------------------------------------------------------------------------------------------- the closed loop
def ref_loop(s, inp, actions=None, dt=torch.float32):
    """ticks x (update_actions from recorded draws and rows, plant step with the first planned action on the nominal model, roll(1));
    actions None: they are formed here, a_seq + sigma_a z around the current sequence, and returned for the other runs"""
    f = cases.FAMILY[s["family"]]
    T = s["ticks"]
    with ms._dtype(dt):
        t = lambda a: torch.as_tensor(np.asarray(a, np.float32)).to(dt)
        ctrl, model, _ = controller(s, dt)
        plant = ref_model(dict(s, up=()))[0]
        ctrl.a_seq = t(inp["a_seq0"]).clone()
        state = t(inp["state"])
        out = {k: [] for k in ("costs", "omega", "a_seq1", "plant", "actions")}
        for k in range(T):
            if actions is None:
                a = (mg.npf(ctrl.a_seq)[None] + np.float32(f["sigma_a"]) * inp["z"][k]).astype(np.float32)
            else:
                a = actions[k]
            feed(model, inp["params"][k], t)
            with torch.no_grad():
                costs, _, _, omega = ctrl.update_actions(model, state, t(a))
                out["actions"].append(a)
                out["costs"].append(mg.npf(costs))
                out["omega"].append(mg.npf(omega))
                out["a_seq1"].append(mg.npf(ctrl.a_seq))
                state = plant.step(state.view(1, -1), ctrl.a_seq[0].view(1, -1)).view(-1)
                out["plant"].append(mg.npf(state))
            ctrl.roll(1)
        return {k: np.stack(v) for k, v in out.items()}


def run_loop(s, write=True):
    inp = cases.loop_inputs(s)
    r32 = ref_loop(s, inp)
    acts = r32["actions"]
    full = dict(inp, actions=acts)
    mv = gc.moved(full, 6000 + s["seed"], ("state", "a_seq0", "actions", "params"))
    rp = ref_loop(s, mv, actions=mv["actions"])
    r64 = ref_loop(s, inp, actions=acts, dt=torch.float64)
    f = cases.FAMILY[s["family"]]
    g = dict(S=s["S"], H=s["H"], P=len(s["up"]), T=s["ticks"], mode=s["mode"], family=s["family"], uncertain=",".join(s["up"]), lam=f["lam"],
             state=inp["state"], a_seq0=inp["a_seq0"], actions=acts, params=inp["params"])
    quant = cases.QUANT + ("plant",)
    bad, row = [], []
    for q in quant:  # per-tick tolerances
        g[q], g[q + "_f64"] = r32[q], r64[q]
        d = np.array([max(elemerr(rp[q][k], r32[q][k]), elemerr(r32[q][k], r64[q][k])) for k in range(s["ticks"])])
        g["tol_" + q] = np.maximum(TOL, 2.0 * d)
        row.append("%s %s" % (q, " ".join("%.1e" % v for v in g["tol_" + q])))
        if g["tol_" + q].max() > CAP:
            bad.append("%s %.1e > cap" % (q, g["tol_" + q].max()))
    re = cases.restate_loop(s, dict(inp, actions=acts))
    for q in quant:
        e = elemerr(re[q], r64[q])
        assert e < 1e-12, (s["tag"], q, e)
    top = float(np.exp(r32["omega"]).max())
    if not top <= 0.5:
        bad.append("top weight %.3f > 0.5" % top)
    # power variants, per tick, from the float64 loop's own sequence and plant state
    power = []
    for v, c in cases.restate_loop_variants(s, dict(inp, actions=acts), r64["a_seq1"], r64["plant"]).items():
        g[v] = c.astype(np.float32)
        p = min(elemerr(g[v][k], g["costs"][k]) / g["tol_costs"][k] for k in range(s["ticks"]))
        power.append("%s %.0f tol" % (v[6:], p))
        if not p >= 10:
            bad.append("power(%s) %.1f tol < 10 tol" % (v, p))
    print("%-15s top %.3f  power %s | %s" % (s["tag"], top, " ".join(power), "  ".join(row)))
    assert not bad or not write, (s["tag"], bad)
    if bad:
        print("   FAILS:", "; ".join(bad))
    if write:
        np.savez_compressed(os.path.join(mg.OUT, "amppi_" + s["tag"] + ".npz"), **g)
    return g


if __name__ == "__main__":
    # --dry: print the tables and write nothing; the fixture's conditions (cap, weight, movement, power) are reported, not asserted.  The
    # restatement's agreement with the float64 run is asserted in either mode: it is a check of tests/amppi_cases.py, not of a fixture.
    dry = "--dry" in sys.argv[1:]
    only = set(sys.argv[1:]) - {"--dry"}
    for s in cases.SCENARIOS:
        if not only or s["tag"] in only:
            run(s, write=not dry)
    if not only or cases.LOOP["tag"] in only:
        run_loop(cases.LOOP, write=not dry)
