"""The skid-steer filter's test scenarios (TEST INFRASTRUCTURE), shared by tests/golden/make_golden_mpf_skid.py, which runs the reference on
them, and by the tests that read the resulting tests/golden/mpf_skid_*.npz.  Data and seeded numpy only: nothing here imports the
reference or the library.

A scenario is a dict:
  tag, up (uncertain parameter names, in column order), Mp, log (GaussianLikelihood(log_space=)), bw, lr, n (steps of a full call),
  obs0 / action (past state and the wheel speeds applied to it), fixed (x_icr, wheel_radius, axial_distance of the model: a sampled
  parameter's entry is unused), lo / hi (wheel-speed bounds), dt, opt ("SGD" / "Adam"), seed, obs_std, spread (relative, log-normal),
  off: what phi0_off ignores (see make_golden_mpf_skid.py).
"""
import numpy as np

NAMES3 = ("x_icr", "wheel_radius", "axial_distance")
DEFAULTS = dict(x_icr=0.2, wheel_radius=0.0625, axial_distance=0.475)  # SkidSteerRobot.__init__
TRUE = dict(x_icr=0.26, wheel_radius=0.07, axial_distance=0.52)         # the plant that makes the observations
OBS_STD, DT = 0.05, 0.1


def particles(up, Mp, log, seed, spread):
    """[Mp, P] fp32 particles: log-normal around the constructor defaults (always positive), as logs when `log`"""
    rng = np.random.default_rng(seed)
    x = np.stack([DEFAULTS[k] * np.exp(spread * rng.standard_normal(Mp)) for k in up], 1)
    return (np.log(x) if log else x).astype(np.float32)


def S(tag, up, Mp, log, bw, lr, n, off, seed, obs0=(0.3, -0.2, 0.7, 0.0, 0.0), action=(0.4, -0.25), fixed=None, lo=(-0.5, -0.5), hi=(0.5, 0.5),
      dt=DT, opt="SGD", spread=None, obs_std=OBS_STD):
    fx = dict(DEFAULTS)
    fx.update(fixed or {})
    return dict(tag=tag, up=tuple(up), Mp=Mp, log=log, bw=bw, lr=lr, n=n, off=off, seed=seed, obs0=tuple(obs0), action=tuple(action), fixed=fx,
                lo=tuple(lo), hi=tuple(hi), dt=dt, opt=opt, spread=(0.2 if log else 0.15) if spread is None else spread, obs_std=obs_std)


XW, WX, A1 = ("x_icr", "wheel_radius"), ("wheel_radius", "x_icr"), ("axial_distance",)
SCENARIOS = [
    S("p3_lin", NAMES3, 130, False, 0.05, 6e-6, 10, dict(log=True), 201),
    S("p3_log", NAMES3, 300, True, 0.3, 1e-4, 10, dict(log=False), 202),
    S("straight", NAMES3, 130, True, 0.3, 2e-4, 10, dict(action=(0.4, -0.25)), 203, action=(0.35, 0.35)),
    S("sat_both", NAMES3, 130, True, 0.3, 2e-4, 10, dict(lo=(-1.0, -1.0), hi=(1.0, 1.0)), 204, action=(0.8, -0.7)),
    S("sat_one", NAMES3, 130, True, 0.3, 2e-4, 10, dict(lo=(-1.0, -1.0), hi=(1.0, 1.0)), 205, action=(0.8, 0.2)),
    S("p2_xw", XW, 70, True, 0.3, 1.5e-4, 10, dict(detach=(1,)), 206),
    S("p2_wx", WX, 70, True, 0.3, 1.5e-4, 10, dict(up=XW), 207),
    S("p1_axial_lin", A1, 600, False, 0.05, 4e-6, 8, dict(drop_last=True), 208),
    S("nondefault", XW, 130, True, 0.3, 2e-4, 10, dict(defaults=True), 209, obs0=(-1.2, 0.8, 7.1, 0.3, -0.9), action=(0.9, -0.3),
      fixed=dict(x_icr=0.1, wheel_radius=0.08, axial_distance=0.6), lo=(-1.0, -0.2), hi=(0.8, 0.6), dt=0.05),
    S("ragged_1021", NAMES3, 1021, True, 0.3, 6e-5, 3, dict(drop_last=True), 210),
    S("adam_130", NAMES3, 130, True, 0.3, 6e-3, 10, dict(action=(0.2, -0.125)), 211, opt="Adam"),
]
NAMES = [s["tag"] for s in SCENARIOS]
BY_TAG = {s["tag"]: s for s in SCENARIOS}

# the size sweep (mpf_skid_sweep.npz): P = 3, log space, every edge of the launch geometry; x0 is rebuilt here, not stored
SWEEP_SIZES = (1, 2, 7, 8, 63, 64, 65, 95, 96, 97, 255, 256, 257, 511, 512, 513, 1023, 1024)


SWEEP_LR_SMALL = {1: 1e-3, 2: 3e-3, 7: 1e-3, 8: 1.2e-3}  # (few particles: phi is small, two steps must still move them by 0.5 % of their rms)


def sweep_scenario(Mp):
    # the repulsion term of phi is a sum over particles: the step size shrinks with their number
    lr = SWEEP_LR_SMALL.get(Mp, 2e-2 / max(Mp, 96))
    return S("sweep_%d" % Mp, NAMES3, Mp, True, 0.3, lr, 2, {}, 4000 + Mp)


def model_kwargs(s):
    """MpfContext keywords of a scenario's model"""
    return dict(model="skid_steer", uncertain_params=s["up"], log_space=s["log"], obs_std=s["obs_std"], dt=s["dt"], min_a=s["lo"], max_a=s["hi"],
                **s["fixed"])
