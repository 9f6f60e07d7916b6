"""Case table of the per-environment filter hyper-parameters (dust_mpf_batch_set_hyper): tests/test_gpu_mpf_sweep.py runs it on the
device, tests/test_mpf_sweep_cpu.py checks the table itself.  numpy only.

A case is a filter configuration (family, particle columns, parameter space, optimiser); a size is a particle count; the rows are the
five kinds a sweep mixes in one batch, B = 5:
  0  the prototype's own values (Silverman's rule, as a call with bw <= 0 without rows)
  1  lr x 4
  2  obs_std x 0.5
  3  bw_scale 0.5 under Silverman's rule
  4  a fixed bandwidth 0.05 beside Silverman neighbours
Every value is a float32 (lr: a float32 widened to double), so that a filter CREATED with a row's values - whose configuration carries
floats - holds the same bits as the row."""
import numpy as np

B = 5
MPF_STEPS = 4
# Mp = 1; 3; 65: the second wave and the padded lanes of the workgroup (Mpad 128); 130: Mpad 192, a block of 768
SIZES = (1, 3, 65, 130)
FIELDS = ("lr", "obs_std", "bw", "bw_scale")

CASES = {
    # family, uncertain parameters (P columns), log space, optimiser
    "pend_sgd": dict(family="pendulum", up=("length", "mass"), log=False, opt="SGD"),
    "pend_p1_sgd": dict(family="pendulum", up=("length",), log=False, opt="SGD"),
    "pend_adam_log": dict(family="pendulum", up=("g", "length", "mass"), log=True, opt="Adam"),  # (the state slots and t0)
    "part_mass_log": dict(family="particle", up=("mass",), log=True, opt="SGD"),
}
# case x size as the GPU tests take them: every size for the two-column SGD case, the edges for the others
GRID = [("pend_sgd", Mp) for Mp in SIZES] + [("pend_p1_sgd", 1), ("pend_p1_sgd", 65), ("pend_adam_log", 3), ("pend_adam_log", 65),
                                              ("pend_adam_log", 130), ("part_mass_log", 1), ("part_mass_log", 65), ("part_mass_log", 130)]
GRID_IDS = ["%s-Mp%d" % g for g in GRID]

CENTRE = dict(length=1.0, mass=1.0, g=9.8)
# (the Particle starts on a FREE cell of the 4 x 4 map, where mpf_part_log.npz starts: on an occupied one - (-3, -3) is - the step's
# Jacobian is zero, the likelihood score with it, and obs_std would change nothing)
STATE0 = dict(pendulum=[3.0, 0.0], particle=[-9.0, -9.0, 0.5, -0.25])


def f32(v):
    return float(np.float32(v))


def proto_row(case):
    """the prototype filter's own values of the four fields (bw 0: Silverman's rule)"""
    # SGD's step is lr x phi: 1e-6 for the Pendulum as in tests/test_gpu_amppi_dual_batch.py; the Particle's mass moves a one-step
    # prediction far less, so its filter takes 1e-3 (the reference's own Particle fixture, mpf_part_log.npz, runs at 1e-2)
    lr = 1e-3 if (CASES[case]["opt"] == "Adam" or CASES[case]["family"] == "particle") else 1e-6
    return dict(lr=f32(lr), obs_std=f32(0.2), bw=0.0, bw_scale=1.0)


def rows(case):
    """the B = 5 rows of the table"""
    p = proto_row(case)
    return [dict(p), dict(p, lr=f32(4.0 * p["lr"])), dict(p, obs_std=f32(0.5 * p["obs_std"])), dict(p, bw_scale=0.5), dict(p, bw=f32(0.05))]


def other_value(case, field):
    """a valid value of `field` that differs from the prototype's: what the 'one field, one environment' test sets"""
    p = proto_row(case)
    return dict(lr=f32(3.0 * p["lr"]), obs_std=f32(0.75 * p["obs_std"]), bw=f32(0.07), bw_scale=0.25)[field]


# one invalid row per invalid field: (field, value)
INVALID = [("lr", 0.0), ("lr", -1e-3), ("lr", float("nan")), ("lr", float("inf")), ("obs_std", 0.0), ("obs_std", float("nan")),
           ("bw_scale", 0.0), ("bw_scale", -0.5), ("bw_scale", float("inf")), ("bw", float("nan")), ("bw", float("inf"))]


def filter_kw(case, row=None):
    """MpfContext's keywords for the case's prototype, or for a filter created with `row`'s obs_std, lr and bw_scale"""
    c = CASES[case]
    r = proto_row(case) if row is None else row
    kw = dict(model=c["family"], uncertain_params=c["up"], obs_std=r["obs_std"], lr=r["lr"], bw_scale=r["bw_scale"], init_bw=0.05,
              optimizer=c["opt"], log_space=c["log"])
    if c["family"] == "particle":
        kw.update(mass=2.0)
    return kw


def particles(case, Mp, env):
    """environment `env`'s first particles [Mp, P] and first observation: its own, whichever slot it sits in"""
    c = CASES[case]
    rng = np.random.default_rng(7000 + 100 * Mp + env)
    centre = np.array([2.0 if (c["family"] == "particle" and k == "mass") else CENTRE[k] for k in c["up"]], np.float32)
    x0 = (centre * (1.0 + 0.05 * rng.standard_normal((Mp, len(c["up"]))))).astype(np.float32)
    s0 = np.array(STATE0[c["family"]], np.float32)
    o0 = (s0 + 0.01 * rng.standard_normal(s0.size)).astype(np.float32)
    return (np.log(x0) if c["log"] else x0).astype(np.float32), o0


def update_inputs(case, env, t, obs_prev):
    """the action and the new observation of environment `env`'s update t"""
    c = CASES[case]
    rng = np.random.default_rng(9000 + 50 * env + t)
    da = 1 if c["family"] == "pendulum" else 2
    act = (0.5 * rng.standard_normal(da)).astype(np.float32)
    return act, (obs_prev + 0.02 * rng.standard_normal(obs_prev.size)).astype(np.float32)
