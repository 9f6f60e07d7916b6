"""Closed-loop episode cases (TEST INFRASTRUCTURE) for dust_svmpc_batch_episode, shared by tests/test_svmpc_episode_cpu.py and
tests/test_gpu_svmpc_episode.py.  Data and seeded numpy only: nothing here imports the library.

A case is an AMPPI scenario dict (tests/amppi_cases.py `A`: family, S, H, the uncertain parameter names in column order), so that the
plant constants of the device context (`amppi_cases.context_kwargs`) and of the float64 restatement (`amppi_cases._step`, imported -
never copied) are the same numbers, plus the SVMPC sizes N, M, n_steps, the periods T, the environments B and the options of the tick.

`plant_tolerance(case)` follows the project's rule (as k2_cases.measure) and is measured from the restatement alone,
on a float64 closed loop of the case's own start states, true rows and seeded actions - never from device output:
d = max(elemerr(step on float32 operands, float64 step), elemerr(step on states moved one fp32 ulp, float64 step)), tol = max(1e-5, 2 d).
`POWER[case]` states, per wrong variant the case can show, the least distance in tolerances that the plant check must keep from it;
`variant_steps` restates the variants (nominal parameters in place of the true row, the previous period's action, the state unstepped).
"""
import numpy as np

import amppi_cases as ac
from helpers import elemerr

TOL_FLOOR, TOL_CAP = 1e-5, 5e-5
NAV = dict(w_obs=10.0, cell_size=0.02)  # the navigation cost of the `skid_nav` case: its map is nav_map()


def _case(tag, family, N, S, M, H, n_steps, T, B, up, seed, opts, scale, true_rel=None, nav=False, start=None):
    return dict(ac.A("episode_" + tag, family, S, H, "extended" if up else "none", up, seed), id=tag, N=N, M=M, n_steps=n_steps, T=T, B=B,
                opts=opts, scale=scale, true_rel=true_rel, nav=nav, start=start)


CASES = [
    # SGD, K1; parameter offsets over t, b, it, m; the true (length, mass) differ per environment
    _case("pend", "pendulum", 3, 16, 3, 6, 2, 3, 3, ("length", "mass"), 1101, dict(kernel="K1", optimizer="SGD", lr=2.0, sigma_p=2.0), 1.0,
          true_rel=((1.25, 0.8), (0.8, 1.2), (1.15, 1.3))),
    # Adam, roll "mean", weighted prior, no uncertain parameters; environment 1 starts inside the obstacle at (-2, -6): the freeze
    _case("part", "particle", 4, 16, 1, 5, 1, 3, 3, (), 1102,
          dict(kernel="K1", optimizer="Adam", lr=1.0, sigma_p=5.0, roll_strategy="mean", weighted_prior=True), 3.0,
          start=((-3.3, -7.3, 4.0, 3.0), (-2.0, -6.0, 1.0, -2.0), (4.4, 0.3, -3.0, 4.5))),
    _case("skid", "skid", 4, 16, 2, 6, 1, 3, 2, ("x_icr",), 1103, dict(kernel="IMQ", optimizer="SGD", lr=0.05, sigma_p=0.3), 0.3,
          true_rel=((1.5,), (0.6,))),
    _case("skid_nav", "skid", 4, 16, 2, 6, 1, 2, 2, ("x_icr",), 1104, dict(kernel="IMQ", optimizer="SGD", lr=0.05, sigma_p=0.3), 0.3,
          true_rel=((1.5,), (0.6,)), nav=True),
    _case("cart", "cartpole", 2, 8, 2, 5, 1, 3, 2, ("mass_pole", "length"), 1105, dict(kernel="K1", optimizer="SGD", lr=0.05, sigma_p=0.5), 0.5,
          true_rel=((2.0, 0.6), (0.5, 1.5))),
    _case("one", "pendulum", 1, 1, 1, 1, 1, 1, 1, (), 1106, dict(kernel="K1", optimizer="SGD", lr=2.0, sigma_p=2.0), 1.0),
]
BY_ID = {c["id"]: c for c in CASES}
IDS = [c["id"] for c in CASES]

# Least distance, in plant tolerances, between the plant's states and each wrong variant over the case's T periods and B environments
# (elemerr of the whole [T, B, ds] record).  A variant a case cannot show is absent: no true row without uncertain parameters (`part`,
# `one`), no previous period at T = 1 (`one`).  The figures are floors, a tenth or less of what the restatement itself shows
# (test_svmpc_episode_cpu.py prints and asserts them): a plant that takes the wrong row, the stale action or no step misses its states
# by hundreds to thousands of tolerances, so 20 separates it from rounding with room on both sides.  Particle's stale action is the one
# weak signal: a unit of action moves a velocity by dt / mass = 0.0075, some 170 tolerances of the record's RMS of 4.5, so its floor is 5.
POWER = {
    "pend": dict(nominal=20.0, prev_action=20.0, unstepped=20.0),
    "part": dict(prev_action=5.0, unstepped=20.0),
    "skid": dict(nominal=20.0, prev_action=20.0, unstepped=20.0),
    "skid_nav": dict(nominal=20.0, prev_action=20.0, unstepped=20.0),
    "cart": dict(nominal=20.0, prev_action=20.0, unstepped=20.0),
    "one": dict(unstepped=20.0),
}


def nav_map():
    """[80, 80] 0 / 1 occupancy in blocks of 2 cells of 0.02 m (200 words: staged into LDS)"""
    rng = np.random.default_rng(7)
    return np.ascontiguousarray(np.kron((rng.random((40, 40)) < 0.4).astype(np.float32), np.ones((2, 2), np.float32)))


def family(case):
    return ac.FAMILY[case["family"]]


def context_kwargs(case, **kw):
    """Context keywords of the case's prototype (the map comes beside them: Context(grid=))"""
    return ac.context_kwargs(case, **dict(dict(N=case["N"], M=case["M"], seed=case["seed"], **(NAV if case["nav"] else {})), **dict(case["opts"], **kw)))


def start_states(case, B=None):
    """[B, ds] fp32: the case's own starts, or the family's operating point shifted per environment"""
    f = family(case)
    B = case["B"] if B is None else B
    if case["start"] is not None:
        return np.asarray(case["start"], np.float32)[:B]
    st = np.asarray(f["state0"], np.float32)
    return np.stack([(st + np.float32(0.05 * b) * np.arange(1, f["ds"] + 1, dtype=np.float32)).astype(np.float32) for b in range(B)])


def nominal_row(case):
    d = family(case)["defaults"]
    return np.array([d[k] for k in case["up"]], np.float32)


def plant_rows(case, B=None):
    """[B, P] fp32 true parameter rows (None without uncertain parameters)"""
    if not case["up"]:
        return None
    B = case["B"] if B is None else B
    return (nominal_row(case)[None] * np.asarray(case["true_rel"], np.float32)[:B]).astype(np.float32)


def tick_params(case, T=None, B=None, seed_shift=0):
    """[T, B, n_steps, M, P] fp32 dynamics samples round the nominal row, every (t, b, it, m) another draw; None without parameters"""
    if not case["up"]:
        return None
    T, B = case["T"] if T is None else T, case["B"] if B is None else B
    rng = np.random.default_rng(case["seed"] + 7 + seed_shift)
    nom = nominal_row(case)
    return (nom * (1.0 + ac.REL_STD * rng.standard_normal((T, B, case["n_steps"], case["M"], len(case["up"]))))).astype(np.float32)


def particles(case, B=None):
    """(prior means, particles) [B, N, H, da] fp32, every environment its own"""
    f = family(case)
    B = case["B"] if B is None else B
    rng = np.random.default_rng(case["seed"] + 3)
    mu = (case["scale"] * rng.standard_normal((B, case["N"], case["H"], f["da"]))).astype(np.float32)
    return mu, (mu + 2 * case["scale"] * rng.standard_normal(mu.shape)).astype(np.float32)


def _pdict(case, rows):
    """name -> Python float or [n, 1] float64 column, as amppi_cases._step reads it; rows [n, P] or None (nominal)"""
    p = dict(family(case)["defaults"])
    if rows is not None:
        for j, k in enumerate(case["up"]):
            p[k] = np.asarray(rows, np.float64)[:, j:j + 1]
    return p


def plant_step(case, x, a, rows, grid=None, dtype=np.float64):
    """states after one plant step: x [n, ds], a [n, da] (raw actions), rows [n, P] true parameter rows or None -> [n, ds] in `dtype`"""
    p = _pdict(case, rows)
    if dtype != np.float64:
        p = {k: (v.astype(dtype) if isinstance(v, np.ndarray) else v) for k, v in p.items()}
    return ac._step(case, np.asarray(x, dtype), np.asarray(a, dtype), p, grid)


def variant_steps(case, x_prev, a, a_before, rows, grid=None):
    """the wrong plants on the same inputs, in float64: {variant: [n, ds]}.  a_before: the previous period's action or None (period 0)"""
    out = dict(unstepped=np.asarray(x_prev, np.float64))
    if rows is not None:
        out["nominal"] = plant_step(case, x_prev, a, np.broadcast_to(nominal_row(case), np.shape(rows)), grid)
    if a_before is not None:
        out["prev_action"] = plant_step(case, x_prev, a_before, rows, grid)
    return out


def restated_loop(case, grid=None):
    """A float64 closed loop of the case from seeded actions: (states [T + 1, B, ds] - the fp32 start, then every stepped state rounded
    to fp32 as the device carries it -, actions [T, B, da] fp32, exact float64 steps [T, B, ds])"""
    f = family(case)
    rng = np.random.default_rng(case["seed"] + 11)
    T, B = case["T"], case["B"]
    acts = (2.0 * f["a_scale"] * rng.standard_normal((T, B, f["da"]))).astype(np.float32)
    rows = plant_rows(case)
    xs, exact = [start_states(case)], []
    for t in range(T):
        exact.append(plant_step(case, xs[-1], acts[t], rows, grid))
        xs.append(exact[-1].astype(np.float32))
    return np.stack(xs), acts, np.stack(exact)


def ulp_moved(x, seed):
    """x (fp32) with every entry moved one ulp up or down"""
    x = np.asarray(x, np.float32)
    up = np.random.default_rng(seed).random(x.shape) < 0.5
    return np.where(up, np.nextafter(x, np.float32(np.inf)), np.nextafter(x, np.float32(-np.inf))).astype(np.float32)


_measured = {}


def measure(cid, grid=None):
    """(d, tol, {variant: distance in tolerances}) of a case from the restatement alone"""
    if cid in _measured:
        return _measured[cid]
    case = BY_ID[cid]
    xs, acts, exact = restated_loop(case, grid)
    rows = plant_rows(case)
    T = acts.shape[0]
    f32 = np.stack([plant_step(case, xs[t], acts[t], rows, grid, dtype=np.float32) for t in range(T)])
    moved = np.stack([plant_step(case, ulp_moved(xs[t], case["seed"] + t), acts[t], rows, grid) for t in range(T)])
    d = max(elemerr(f32, exact), elemerr(moved, exact))
    tol = max(TOL_FLOOR, 2.0 * d)
    var = {}
    for t in range(T):
        for k, v in variant_steps(case, xs[t], acts[t], acts[t - 1] if t else None, rows, grid).items():
            var.setdefault(k, []).append(v)
    # (a variant is judged on the periods that have it: `prev_action` from period 1 on)
    power = {k: elemerr(np.stack(v), exact[T - len(v):]) / tol for k, v in var.items()}
    _measured[cid] = (d, tol, power)
    return _measured[cid]


def plant_tolerance(case, grid=None):
    d, tol, _ = measure(case["id"], grid)
    assert tol <= TOL_CAP, (case["id"], d)
    return tol
