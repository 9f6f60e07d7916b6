"""The cart-pole family's test scenarios (TEST INFRASTRUCTURE), shared by tests/golden/make_golden_cartpole.py and
make_golden_mpf_cartpole.py, which run the reference on them, and by the tests that read the resulting tests/golden/cartpole_*.npz and
mpf_cartpole_*.npz.  Data and seeded numpy only: nothing here imports the reference or the library.

Controller scenarios (ROLLOUTS, TICKS) are dicts:
  tag, N, S, H, M, up (uncertain parameter names, in column order; () = nominal), dist ("uniform" / "lognormal" / "scalar" / None) with
  lo / hi or loc / scale per column, log (params_log_space), fixed (the seven constructor values), off: what costs_off ignores
  ("clamp" / "mass" / "mu_c" / "mu_p" / "interleave" / "areg"), seed, optionally ctrl_penalty (1.0) and a_seq (a non-zero a_seq0 is set on the
  controller); TICKS add kernel ("K1" / "K2"), opt ("SGD" / "Adam"), lr, alpha.
Filter scenarios (SCENARIOS, sweep_scenario) follow tests/mpf_skid_cases.py:
  tag, up, Mp, log, bw, lr, n, obs0 / action (past state and the push applied to it), fixed, dt, opt, seed, obs_std, spread, off: what
  phi0_off ignores (see make_golden_mpf_cartpole.py).
"""
import numpy as np

NAMES7 = ("g", "mass_cart", "mass_pole", "length", "mu_c", "mu_p", "f_mag")  # params_dict order of CartPoleModel (cartpole.py:79-87)
DEFAULTS = dict(g=9.8, mass_cart=1.0, mass_pole=0.1, length=1.0, mu_c=0.5e-3, mu_p=2e-6, f_mag=10.0)  # CartPoleModel.__init__
# with the constructor's frictions neither friction term moves a cost by ten tolerances: fixtures about them use these
FRICTION = dict(mu_c=0.05, mu_p=0.01)
TRUE = dict(g=9.8, mass_cart=1.2, mass_pole=0.13, length=0.9, mu_c=0.06, mu_p=0.012, f_mag=9.0)  # the plant that makes the observations
OBS_STD, DT = 0.05, 0.05

# the quadratic cost of every controller scenario (dust_amd.costs.QuadraticCost), the start state and the noise scale
GOAL = (0.0, 0.0, 0.0, 0.0)
W_STATE = (0.5, 0.05, 2.0, 0.05)
W_TERM = (2.0, 0.2, 8.0, 0.2)
W_CTRL = (0.1,)
STATE0 = (0.1, 0.2, 0.15, -0.1)   # (x_d != 0: see make_golden_cartpole.py)
SIGMA_A = 0.6          # around a_mat of scale 0.5: about a fifth of the actions lie beyond the step's +-1 clamp
TEMPERATURE = 4.0


def _fx(**over):
    d = dict(DEFAULTS)
    d.update(over)
    return d


def R(tag, N, S, H, M, up, dist, off, seed, log=False, fixed=None, **kw):
    return dict(tag=tag, N=N, S=S, H=H, M=M, up=tuple(up), dist=dist, off=off, seed=seed, log=log, fixed=_fx(**(fixed or {})), **kw)


ROLLOUTS = [
    R("nominal", 6, 16, 10, 1, (), None, "clamp", 31),
    R("params", 6, 16, 10, 3, ("mass_cart", "mass_pole", "length"), "uniform", "mass", 32, lo=(0.8, 0.08, 0.8), hi=(1.3, 0.14, 1.2)),
    R("params_log", 6, 16, 10, 4, ("length", "f_mag", "g", "mu_p"), "lognormal", "mu_p", 33, log=True, fixed=FRICTION,
      loc=(0.0, 2.3, 2.28, -4.6), scale=(0.1, 0.1, 0.05, 0.2)),
    # 37 x 9 = 333 lanes: one full 256-lane block and a partial one; D = 31 is odd
    R("ragged", 37, 9, 31, 2, ("mu_c", "f_mag"), "uniform", "mu_c", 34, fixed=FRICTION, lo=(0.03, 8.0), hi=(0.08, 12.0)),
    # a scalar-event params_dist: rollout r uses params[r % M] (disco.py:177-179); N S = 77 is no multiple of M = 3
    R("scalar", 7, 11, 10, 3, ("length",), "scalar", "interleave", 35, loc=(1.0,), scale=(0.15,)),
    # ctrl_penalty != 1: the control-regularisation term of disco.py:338-346, around a non-zero a_seq0 (otherwise `params`)
    R("areg", 6, 16, 10, 3, ("mass_cart", "mass_pole", "length"), "uniform", "areg", 36, lo=(0.8, 0.08, 0.8), hi=(1.3, 0.14, 1.2), ctrl_penalty=0.6,
      a_seq=True),
]
ROLLOUT_NAMES = [s["tag"] for s in ROLLOUTS]
ROLLOUT_BY_TAG = {s["tag"]: s for s in ROLLOUTS}
ROLLOUT_QUANT = ("costs", "states", "omega", "a_mat1", "a_mix")


TWIN_SCALE = 65536.0


def twin(g, q):
    """The float64 twin of a fixture's quantity q.  Stored whole as `q_f64`, or - the rollouts' states, the bulk of those files - as
    `q_f64_delta16`: its difference from the fp32 value, taken in float64, times TWIN_SCALE, in binary16.  The difference is some 1e-7
    of a state and binary16 keeps 11 bits of it (TWIN_SCALE lifts it into the normal range): the twin comes back to 1e-10 of a state."""
    if q + "_f64" in g:
        return g[q + "_f64"]
    return g[q].astype(np.float64) + g[q + "_f64_delta16"].astype(np.float64) / TWIN_SCALE


def lead_quantity(s):
    """the quantity whose `_off` variant a rollout fixture carries"""
    return "states" if s["off"] == "interleave" else "costs"

TICKS = [
    R("tick_k1_sgd", 8, 16, 12, 3, ("mass_pole", "length"), "uniform", "mass", 41, lo=(0.08, 0.8), hi=(0.14, 1.2), kernel="K1", opt="SGD", lr=0.05,
      alpha=0.25),
    R("tick_k2", 8, 16, 12, 3, ("mass_pole", "length"), "uniform", "clamp", 42, lo=(0.08, 0.8), hi=(0.14, 1.2), kernel="K2", opt="SGD", lr=0.05,
      alpha=0.25),
    R("tick_k1_adam", 8, 16, 12, 3, ("mu_c", "f_mag"), "uniform", "mu_c", 43, fixed=FRICTION, lo=(0.03, 8.0), hi=(0.08, 12.0), kernel="K1", opt="Adam",
      lr=0.01, alpha=0.25),
    # tick_k1_sgd with ctrl_penalty != 1: every iteration's costs carry the term, through the a_mat the iteration before left
    R("tick_areg", 8, 16, 12, 3, ("mass_pole", "length"), "uniform", "areg", 44, lo=(0.08, 0.8), hi=(0.14, 1.2), kernel="K1", opt="SGD", lr=0.05,
      alpha=0.25, ctrl_penalty=0.6),
]
TICK_NAMES = [s["tag"] for s in TICKS]
TICK_BY_TAG = {s["tag"]: s for s in TICKS}
TICK_ITERS = 2
TICK_QUANT = ("costs", "score", "phi", "theta_after", "log_l", "log_p", "p_weights")


def controller_kwargs(s, **kw):
    """Context keywords of a controller scenario"""
    d = dict(model="cartpole", N=s["N"], S=s["S"], M=s["M"], H=s["H"], dt=DT, sigma_a=SIGMA_A, sigma_p=SIGMA_A, temperature=TEMPERATURE,
             alpha=1.0 / TEMPERATURE, ctrl_penalty=s.get("ctrl_penalty", 1.0), uncertain_params=s["up"] or None, params_log_space=s["log"], params_scalar_event=s["dist"] == "scalar",
             goal=GOAL, w_quad_state=W_STATE, w_quad_term=W_TERM, w_quad_ctrl=W_CTRL, **s["fixed"])
    d.update(kw)
    return d


# ------------------------------------------------------------------------------------------------ the filter
def particles(up, Mp, log, seed, spread, centre=None):
    """[Mp, P] fp32 particles: log-normal around the constructor defaults (the larger frictions for mu_c / mu_p; `centre` overrides), as
    logs when `log`"""
    rng = np.random.default_rng(seed)
    centre = dict(_fx(**FRICTION), **(centre or {}))
    x = np.stack([centre[k] * np.exp(spread * rng.standard_normal(Mp)) for k in up], 1)
    return (np.log(x) if log else x).astype(np.float32)


def S(tag, up, Mp, log, bw, lr, n, off, seed, obs0=(0.3, 0.5, 0.4, -0.8), action=(0.6,), fixed=None, dt=DT, opt="SGD", spread=None, obs_std=OBS_STD,
      centre=None):
    return dict(centre=centre, tag=tag, up=tuple(up), Mp=Mp, log=log, bw=bw, lr=lr, n=n, off=off, seed=seed, obs0=tuple(obs0), action=tuple(action),
                fixed=_fx(**(fixed or {})), dt=dt, opt=opt, spread=(0.2 if log else 0.15) if spread is None else spread, obs_std=obs_std)


P3 = ("mass_cart", "length", "f_mag")
P3L = ("mass_cart", "mass_pole", "length")  # (linear space: columns of one scale, as the one bandwidth asks)
P4 = ("g", "length", "mu_c", "f_mag")
PF = ("mu_p", "mu_c", "mass_pole", "mass_cart")
LM, ML = ("length", "mass_pole"), ("mass_pole", "length")
SCENARIOS = [
    S("p3_lin", P3L, 130, False, 0.1, 3e-4, 6, dict(log=True), 301),
    S("p4_log", P4, 300, True, 0.3, 1e-4, 10, dict(log=False), 302, fixed=FRICTION),
    S("fric_log", PF, 130, True, 0.4, 2e-4, 10, dict(detach=(0,)), 303, fixed=FRICTION, obs0=(0.3, 0.5, 0.4, -4.0), centre=dict(mu_p=0.05, mu_c=0.3)),
    S("sat", P3, 130, True, 0.3, 2e-4, 10, dict(noclamp=True), 304, action=(1.7,)),
    S("xd_zero", P4, 130, True, 0.3, 2e-4, 10, dict(obs0=(0.3, 0.4, 0.4, -0.8)), 305, fixed=FRICTION, obs0=(0.3, 0.0, 0.4, -0.8)),
    S("p2_lm", LM, 70, True, 0.3, 2.5e-4, 10, dict(detach=(0,)), 306),
    S("p2_ml", ML, 70, True, 0.3, 4e-4, 10, dict(up=LM), 307),
    S("p1_length_600", ("length",), 600, False, 0.1, 4e-5, 8, dict(drop_last=True), 308),
    S("ragged_1021", P3, 1021, True, 0.3, 6e-5, 3, dict(drop_last=True), 310),
    S("adam_130", P3, 130, True, 0.3, 6e-3, 10, dict(action=(0.3,)), 311, opt="Adam"),
    S("nondefault", LM, 130, True, 0.3, 2e-4, 10, dict(defaults=True), 309, obs0=(-1.2, -0.7, 2.6, 1.1), action=(-0.8,),
      fixed=dict(g=9.5, mass_cart=1.4, mass_pole=0.2, length=0.7, mu_c=0.03, mu_p=0.02, f_mag=8.0), dt=0.02),
]
NAMES = [s["tag"] for s in SCENARIOS]
BY_TAG = {s["tag"]: s for s in SCENARIOS}

# the size sweep (mpf_cartpole_sweep.npz): P = 3, log space, the sizes of the skid-steer sweep (every edge of the launch geometry)
from mpf_skid_cases import SWEEP_SIZES  # noqa: E402,F401
SWEEP_LR_SMALL = {1: 6e-3, 2: 3e-3, 7: 1e-3, 8: 1.2e-3}  # (few particles: phi is small, two steps must still move them by 0.5 % of their rms)


def sweep_scenario(Mp):
    # the repulsion term of phi is a sum over particles: the step size shrinks with their number
    lr = SWEEP_LR_SMALL.get(Mp, 2e-2 / max(Mp, 96))
    return S("sweep_%d" % Mp, P3, Mp, True, 0.3, lr, 2, {}, 5000 + Mp)


def model_kwargs(s):
    """MpfContext keywords of a scenario's model"""
    return dict(model="cartpole", uncertain_params=s["up"], log_space=s["log"], obs_std=s["obs_std"], dt=s["dt"], **s["fixed"])
