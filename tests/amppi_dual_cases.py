"""Scenarios of the AMPPI dual-loop fixtures (tests/golden/amppi_dual_<tag>.npz, made by tests/golden/make_golden_amppi_dual.py from the
reference's own MPF.optimize and AMPPI.update_actions, composed as its simulation loop composes filter and controller).  Data and numpy
only: the generator and the tests read it.  The controller half of a period is restated by tests/amppi_cases.py `restate` (float64)."""
import numpy as np

import amppi_cases as ac

TICKS = 4
QUANT = ("costs", "omega", "a_seq1", "x", "bw")
TOL, CAP = ac.TOL, ac.CAP


def D(tag, family, mode, up, S, H, Mp, bw, seed, **kw):
    d = dict(tag=tag, family=family, mode=mode, up=tuple(up), S=S, H=H, Mp=Mp, bw=bw, seed=seed, mpf_steps=5, states=False)
    d.update(kw)
    return d


# the filter's settings per family: observation noise, SGD step, particle spread, the plant's true parameters
FILTER = dict(pendulum=dict(obs_std=0.1, lr=3e-4, spread=0.15, centre=dict(length=1.0, mass=1.0)),
              particle=dict(obs_std=0.02, lr=2e-3, spread=0.3, centre=dict(mass=2.0)),
              # (the plant is the model with its default parameters; the particles start 15 % above them)
              skid=dict(obs_std=0.05, lr=3e-6, spread=0.1, centre=dict(wheel_radius=0.085), relative=True),
              cartpole=dict(obs_std=0.05, lr=1e-5, spread=0.02, centre=dict(mass_pole=0.115, length=1.15)))
# the plant's parameters (cart-pole: the model's defaults)
TRUE = dict(pendulum=dict(g=9.8, length=0.8, mass=1.25), particle=dict(mass=3.0))
SCENARIOS = [
    D("pend_ext", "pendulum", "extended", ("length", "mass"), 64, 8, 16, None, 212),   # bw None: Silverman's rule of the particles
    D("part_ext", "particle", "extended", ("mass",), 64, 10, 16, 0.1, 221),
    D("cart_single", "cartpole", "single", ("mass_pole", "length"), 64, 8, 16, 0.02, 231),
    # the sigma points of the filter's prior over wheel_radius alone: the filter starts 36 % off the plant's value and closes part of the gap
    # every period, so that the points of the prior BEFORE the update (costs_stale) lie visibly elsewhere
    D("skid_ut", "skid", "ut", ("wheel_radius",), 64, 7, 16, 0.03, 257, mpf_steps=10),
]
NAMES = [s["tag"] for s in SCENARIOS]
BY_TAG = {s["tag"]: s for s in SCENARIOS}
VARIANTS = ("disco", "noctrl", "single", "stale")


def variants_of(s):
    if s["mode"] == "ut":
        return ("disco", "noctrl", "mean", "stale")
    return tuple(v for v in VARIANTS if v != "single" or s["mode"] == "extended")


def inputs(s):
    """start state, start sequence, the filter's particles and the standard-normal action draws of every period, fp32, seeded"""
    f, flt = ac.FAMILY[s["family"]], FILTER[s["family"]]
    rng = np.random.default_rng(s["seed"])
    centre = np.array([flt["centre"][k] for k in s["up"]], np.float32)
    x0 = centre * (1.0 + np.float32(flt["spread"]) * rng.standard_normal((s["Mp"], len(s["up"])))) if flt.get("relative") else \
        centre + np.float32(flt["spread"]) * rng.standard_normal((s["Mp"], len(s["up"])))
    x0 = (np.maximum(x0, 0.3) if s["family"] in ("pendulum", "particle") else x0).astype(np.float32)
    return dict(state=np.array(f["state0"], np.float32), a_seq0=(f["a_scale"] * rng.standard_normal((s["H"], f["da"]))).astype(np.float32),
                x0=x0, z=rng.standard_normal((TICKS, s["S"], s["H"], f["da"])).astype(np.float32))


def tick_input(g, k, a_seq, state, rows=None):
    """the controller half of period k as amppi_cases.restate reads it"""
    d = dict(state=state, a_seq0=a_seq, actions=g["actions"][k])
    if "params" in g:
        d["params"] = g["params"][k] if rows is None else rows
    return d


def restate_costs(s, g, k, variant, f64=True):
    """float64 costs of period k from the reference's own sequence and plant state of that period; variant: None, one of amppi_cases's, or
    "stale" - the rows drawn from the prior BEFORE the filter update that opened the period (k >= 1)"""
    sfx = "_f64" if f64 else ""
    a_seq = g["a_seq0"].astype(np.float64) if k == 0 else np.concatenate([g["a_seq1" + sfx][k - 1][1:], np.zeros_like(g["a_seq0"][:1], np.float64)])
    state = g["state"].astype(np.float64) if k == 0 else g["plant" + sfx][k - 1].astype(np.float64)
    if s["mode"] == "ut":  # (the stale points of period k are the points of period k - 1: the prior changes in the filter update alone)
        sp = g["sigma_points" + sfx][k - 1 if variant == "stale" else k]  # (fp32 values in either run, utf.py:108-118, each run its own)
        return ac.restate(s, tick_input(g, k, a_seq, state), variant=None if variant == "stale" else variant, sigma_points=sp)
    rows = g["params_stale"][k] if variant == "stale" else None
    return ac.restate(s, tick_input(g, k, a_seq, state, rows), variant=None if variant == "stale" else variant, grid=grid_of(s))


def grid_of(s):
    if s["family"] != "particle":
        return None
    from oracle import grid_4x4_map

    return grid_4x4_map()


def restate_plant(s, g, k):
    """float64 plant state after period k: one step of the model with the plant's parameters from the previous plant state (the fp32 start
    state in period 0) under the first row of the float64 run's updated sequence"""
    f = ac.FAMILY[s["family"]]
    prev = np.asarray(g["state"], np.float32).astype(np.float64) if k == 0 else g["plant_f64"][k - 1]
    p = dict(f["defaults"], **TRUE.get(s["family"], {}))
    return ac._step(dict(s, mode="none"), prev[None], g["a_seq1_f64"][k][:1], p, grid_of(s))[0]


def restate_bw(s, g, k):
    """the bandwidth of period k's filter update: the fixed one, or Silverman's rule of the particles the update started from (mpf.py:68-73,
    with the project's restatement of KDEpy's rule - the one the generator's shim hands the reference)"""
    if s["bw"] is not None:
        return float(s["bw"])
    from dust_amd.inference.mpf import silvermans_rule

    x = g["x0"].astype(np.float64) if k == 0 else g["x_f64"][k - 1]
    return silvermans_rule(x.reshape(-1, 1))
