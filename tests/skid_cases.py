"""The skid-steer controller's test scenarios (TEST INFRASTRUCTURE), shared by tests/golden/make_golden_skid.py, which runs the reference
on them, and by the tests that read the resulting tests/golden/skid_ctrl_<tag>.npz.  Data and seeded numpy only: nothing here imports
the reference or the library.  The pattern is tests/cartpole_cases.py's.

Scenarios (ROLLOUTS) are dicts:
  tag, N, S, H, M, up (uncertain parameter names, in column order; () = nominal), dist ("uniform" / "lognormal" / "scalar" / None) with
  lo / hi or loc / scale per column, log (params_log_space), fixed (x_icr, wheel_radius, axial_distance), bounds (wheel-speed lo, hi), dt,
  a_cov (None: SIGMA_A^2 I, or a full 2 x 2), act_scale (scale of a_mat0 and of the noise around it, in units of SIGMA_A),
  ctrl_penalty, a_seq (a non-zero a_seq0 is set on the controller), calls (consecutive forward calls, each on fresh actions and draws),
  off: what the `_off` variant of the lead quantity ignores, seed.
Every recorded array has a leading axis over the calls (length 1 or 2).
"""
import numpy as np

NAMES3 = ("x_icr", "wheel_radius", "axial_distance")  # params_dict order of SkidSteerRobot (skid_steer_robot.py:39-43)
DEFAULTS = dict(x_icr=0.2, wheel_radius=0.0625, axial_distance=0.475)  # SkidSteerRobot.__init__
BOUNDS = (-0.5, 0.5)
DT = 0.1

# the quadratic cost, the start state and the noise scale of tests/golden/make_golden_r3.py
GOAL = (1.0, 0.5, 0.3, 0.0, 0.0)
W_STATE = (2.0, 2.0, 0.5, 0.1, 0.05)
W_TERM = (50.0, 50.0, 5.0, 0.0, 0.0)
W_CTRL = (0.3, 0.2)
STATE0 = (0.3, -0.2, 0.4, 0.1, -0.05)
SIGMA_A = 0.3
TEMPERATURE = 0.8
FULL_COV = ((0.09, 0.03), (0.03, 0.0625))
CTRL_PENALTY = 0.6


def R(tag, N, S, H, M, up, dist, off, seed, log=False, fixed=None, bounds=BOUNDS, dt=DT, a_cov=None, act_scale=1.0, ctrl_penalty=1.0, a_seq=False,
      calls=1, **kw):
    return dict(tag=tag, N=N, S=S, H=H, M=M, up=tuple(up), dist=dist, off=off, seed=seed, log=log, fixed=dict(DEFAULTS, **(fixed or {})),
                bounds=tuple(bounds), dt=dt, a_cov=a_cov, act_scale=act_scale, ctrl_penalty=ctrl_penalty, a_seq=a_seq, calls=calls, **kw)


XW = dict(lo=(0.1, 0.05), hi=(0.3, 0.08))  # the (x_icr, wheel_radius) box of skid_params
ROLLOUTS = [
    # 37 x 9 = 333 lanes: one full 256-lane block and a partial one; D = 30: the last Philox block of a row is partial
    R("ragged", 37, 9, 15, 2, ("wheel_radius", "x_icr"), "uniform", "order", 61, lo=(0.05, 0.1), hi=(0.08, 0.3)),
    R("p3_log", 6, 16, 10, 4, ("axial_distance", "x_icr", "wheel_radius"), "lognormal", "exp_ad", 62, log=True, loc=(-0.75, -1.6, -2.8),
      scale=(0.1, 0.2, 0.1)),
    # a scalar-event params_dist: rollout r uses params[r % M] (disco.py:177-179); N S = 77 is no multiple of M = 3
    R("scalar", 7, 11, 10, 3, ("axial_distance",), "scalar", "interleave", 63, loc=(0.475,), scale=(0.08,)),
    R("bounds", 6, 16, 10, 1, (), None, "clamp", 64, fixed=dict(x_icr=0.1, wheel_radius=0.08, axial_distance=0.6), bounds=(-1.0, 0.8), dt=0.05,
      act_scale=2.5),
    R("fullcov", 6, 16, 10, 3, ("x_icr", "wheel_radius"), "uniform", "chol_off", 65, a_cov=FULL_COV, **XW),
    R("areg", 6, 16, 10, 3, ("x_icr", "wheel_radius"), "uniform", "areg", 66, ctrl_penalty=CTRL_PENALTY, a_seq=True, **XW),
    R("areg_fullcov", 6, 16, 10, 3, ("x_icr", "wheel_radius"), "uniform", "apre_off", 67, a_cov=FULL_COV, ctrl_penalty=CTRL_PENALTY, a_seq=True, **XW),
    R("areg_two", 6, 16, 10, 3, ("x_icr", "wheel_radius"), "uniform", "areg2", 68, ctrl_penalty=CTRL_PENALTY, a_seq=True, calls=2, **XW),
]
ROLLOUT_NAMES = [s["tag"] for s in ROLLOUTS]
ROLLOUT_BY_TAG = {s["tag"]: s for s in ROLLOUTS}
ROLLOUT_QUANT = ("costs", "states", "omega", "a_mat1", "a_mix")  # cartpole_cases.ROLLOUT_QUANT

TWIN_SCALE = 65536.0


def twin(g, q):
    """The float64 twin of a fixture's quantity q: stored whole as `q_f64`, or - the states - as `q_f64_delta16` (cartpole_cases.twin)"""
    if q + "_f64" in g:
        return g[q + "_f64"]
    return g[q].astype(np.float64) + g[q + "_f64_delta16"].astype(np.float64) / TWIN_SCALE


def lead_quantity(s):
    """the quantity whose `_off` variant a fixture carries"""
    return "states" if s["off"] == "interleave" else "costs"


def a_cov_of(s):
    return np.asarray(s["a_cov"] if s["a_cov"] is not None else ((SIGMA_A ** 2, 0.0), (0.0, SIGMA_A ** 2)), np.float64)


def controller_kwargs(s, **kw):
    """Context keywords of a scenario"""
    d = dict(model="skid_steer", N=s["N"], S=s["S"], M=s["M"], H=s["H"], dt=s["dt"], sigma_a=SIGMA_A, sigma_p=SIGMA_A, temperature=TEMPERATURE,
             alpha=1.0 / TEMPERATURE, ctrl_penalty=s["ctrl_penalty"], uncertain_params=s["up"] or None, params_log_space=s["log"],
             params_scalar_event=s["dist"] == "scalar", min_a=s["bounds"][0], max_a=s["bounds"][1], goal=GOAL, w_quad_state=W_STATE,
             w_quad_term=W_TERM, w_quad_ctrl=W_CTRL, **s["fixed"])
    if s["a_cov"] is not None:
        d["a_cov"] = np.asarray(s["a_cov"], np.float32)
    d.update(kw)
    return d
