"""Dual-loop episode cases (TEST INFRASTRUCTURE) for dust_svmpc_dual_batch_episode, shared by tests/test_svmpc_dual_episode_cpu.py and
tests/test_gpu_svmpc_dual_episode.py.  Data and seeded numpy only: nothing here imports the library.

A case is an episode case of tests/svmpc_episode_cases.py (`_case`: an AMPPI scenario dict plus the SVMPC sizes), so that the plant
constants of the device context and of the float64 restatement (`svmpc_episode_cases.plant_step`, imported - never copied) are the same
numbers, plus the filter side: Mp particles, `mpf_steps` steps per update, `mpf_bw` (None: Silverman's rule), the filter's optimiser and
space, and `first` (the call hands actions_prev: period 0 updates too).

In every case the TRUE parameter rows differ from the nominal ones by 10 - 40 %, another factor per environment, and the start state
moves (Pendulum [3, 0]: falling; Particle away from its target, with speed): no filter update is a fixed point, so a stale observation, a
stale action or a stale step count changes bits.

The plant check's tolerance is `svmpc_episode_cases.plant_tolerance` of the family's case THERE (`pend`, `part`): measured from the
restatement alone and not re-tuned here.  FACTOR: every wrong plant of `svmpc_episode_cases.variant_steps` lies at least that many
tolerances from the right one in at least one period (tests/test_svmpc_dual_episode_cpu.py proves it on a restated loop).
"""
import numpy as np

import svmpc_episode_cases as ec

FACTOR = 5.0


def _case(tag, family, N, S, M, H, n_steps, T, B, up, seed, opts, scale, true_rel, Mp, mpf_steps, mpf_bw, filt_opt, log=False, first=False,
          start=None):
    c = ec._case(tag, family, N, S, M, H, n_steps, T, B, up, seed, dict(opts, params_log_space=log), scale, true_rel=true_rel, start=start)
    c.update(Mp=Mp, mpf_steps=mpf_steps, mpf_bw=mpf_bw, filt_opt=filt_opt, log=log, first=first)
    return c


PEND_START = ((3.0, 0.0),) * 5
CASES = [
    # the common path: SGD on both sides, Silverman's rule per period on the device
    _case("pend_sgd_silverman", "pendulum", 3, 8, 3, 5, 1, 4, 3, ("length", "mass"), 2101, dict(kernel="K1", optimizer="SGD", lr=2.0, sigma_p=2.0),
          1.0, ((1.25, 0.8), (0.8, 1.2), (1.15, 1.3)), 48, 3, None, "SGD", start=PEND_START),
    # Adam reads t0 (bias correction); Mp = 65 leaves the padded width; n_steps > 1 draws rows it M + m
    _case("pend_adam_fixed", "pendulum", 4, 16, 8, 6, 3, 5, 2, ("g", "mass", "length"), 2102, dict(kernel="IMQ", optimizer="Adam", lr=0.5, sigma_p=2.0),
          1.0, ((0.85, 1.3, 0.75), (1.2, 0.7, 1.35)), 65, 2, 0.3, "Adam", start=PEND_START),
    # the call hands actions_prev: period 0 updates; log space on both sides (plant_params are logarithms)
    _case("pend_log_first_update", "pendulum", 2, 4, 1, 3, 2, 3, 2, ("length",), 2103, dict(kernel="K1", optimizer="SGD", lr=2.0, sigma_p=2.0),
          1.0, ((1.3,), (0.7,)), 3, 2, None, "SGD", log=True, first=True, start=PEND_START),
    # ds = 4, da = 2; environment 1 starts ON an occupied cell of the 4 x 4 grid, (-2, -6): the collision freeze holds its whole state
    _case("part_mass_grid", "particle", 3, 8, 4, 4, 1, 4, 3, ("mass",), 2104,
          dict(kernel="K1", optimizer="SGD", lr=100.0, sigma_p=5.0, roll_strategy="mean", weighted_prior=True), 3.0, ((1.3,), (0.75,), (0.85,)),
          48, 2, 0.5, "SGD", start=((-3.3, -7.3, 4.0, 3.0), (-2.0, -6.0, 1.0, -2.0), (4.4, 0.3, -3.0, 4.5))),
    # every loop bound at 1; no actions_prev and T = 1: no filter launch at all
    _case("ones", "pendulum", 1, 1, 1, 1, 1, 1, 1, ("length",), 2105, dict(kernel="K1", optimizer="SGD", lr=2.0, sigma_p=2.0), 1.0, ((1.3,),),
          1, 1, 0.1, "SGD", start=PEND_START),
]
BY_ID = {c["id"]: c for c in CASES}
IDS = [c["id"] for c in CASES]
FROZEN = {"part_mass_grid": 1}  # the environment that starts on an occupied cell


def tolerance_case(case):
    """the case of tests/svmpc_episode_cases.py whose measured plant tolerance holds for this family"""
    return ec.BY_ID["pend" if case["family"] == "pendulum" else "part"]


def plant_tolerance(case, grid=None):
    return ec.plant_tolerance(tolerance_case(case), grid)


def true_rows(case, B=None):
    """[B, P] fp32 true parameter rows, in natural units (the float64 restatement reads these)"""
    return ec.plant_rows(case, B)


def device_rows(case, B=None):
    """... in the space of the controller's dynamics samples (what plant_params takes)"""
    r = true_rows(case, B)
    return np.log(r).astype(np.float32) if case["log"] else r


def filter_particles(case, B=None):
    """[B, Mp, P] fp32 filter particles round the NOMINAL row (5 % spread), every environment its own, in the filter's space"""
    B = case["B"] if B is None else B
    rng = np.random.default_rng(case["seed"] + 5)
    x = (ec.nominal_row(case) * (1.0 + 0.05 * rng.standard_normal((B, case["Mp"], len(case["up"]))))).astype(np.float32)
    return np.log(x).astype(np.float32) if case["log"] else x


def first_actions(case, B=None):
    """[B, da] fp32: the call's actions_prev of a `first` case (None otherwise)"""
    if not case["first"]:
        return None
    B = case["B"] if B is None else B
    f = ec.family(case)
    return (f["a_scale"] * np.random.default_rng(case["seed"] + 9).standard_normal((B, f["da"]))).astype(np.float32)


def prior_seeds(case, T=None, B=None):
    """[T, B] uint64 Philox keys, every (period, environment) another"""
    T, B = case["T"] if T is None else T, case["B"] if B is None else B
    return (np.uint64(case["seed"]) * np.uint64(1000003) + (np.arange(B, dtype=np.uint64)[None] << np.uint64(32))
            + np.arange(1, T + 1, dtype=np.uint64)[:, None])


def stand_in_actions(case, xs_t, t):
    """A deterministic stand-in controller for the restated loop: a bounded feedback on the state plus a term that alternates with the
    period, so that successive actions differ and stay inside the plants' clamps -> [B, da] fp32"""
    f = ec.family(case)
    x = np.asarray(xs_t, np.float64)
    base = np.tanh(0.3 * x[:, : f["da"]] + 0.2 * x[:, -f["da"]:])
    swing = (0.6 if t % 2 == 0 else -0.5) + 0.1 * t
    lim = np.minimum(np.abs(np.asarray(f["lo"], np.float64)), np.abs(np.asarray(f["hi"], np.float64)))
    return (0.5 * lim * (base + swing)).astype(np.float32)


def restated_loop(case, grid=None):
    """The float64 closed loop of the case under its true rows and the stand-in controller: (states [T + 1, B, ds] fp32 as the device
    carries them, actions [T, B, da] fp32, exact float64 steps [T, B, ds])"""
    rows = true_rows(case)
    xs, acts, exact = [ec.start_states(case)], [], []
    for t in range(case["T"]):
        acts.append(stand_in_actions(case, xs[-1], t))
        exact.append(ec.plant_step(case, xs[-1], acts[-1], rows, grid))
        xs.append(exact[-1].astype(np.float32))
    return np.stack(xs), np.stack(acts), np.stack(exact)


def variant_distances(case, prev, acts, xs, tol, grid=None):
    """{variant: the largest distance over the periods, in tolerances, between the recorded states xs [T, B, ds] and that wrong plant on
    the same inputs (prev [T, B, ds]: the state each period started from)}.  A period is judged on its own: elemerr of its [B, ds]."""
    from helpers import elemerr

    rows, far = true_rows(case), {}
    for t in range(acts.shape[0]):
        for k, v in ec.variant_steps(case, prev[t], acts[t], acts[t - 1] if t else None, rows, grid).items():
            far[k] = max(far.get(k, 0.0), elemerr(xs[t], v) / tol)
    return far
