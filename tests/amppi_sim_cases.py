"""Cases (TEST INFRASTRUCTURE) for dust_amppi_batch_simulate / dust_amppi_dual_batch_simulate - the AMPPI episodes under the reference's
rules: the accumulated cost, crash and goal -, shared by tests/test_amppi_sim_cpu.py, tests/test_gpu_amppi_sim.py and
tests/test_gpu_amppi_dual_sim.py.  Data and seeded numpy only: nothing here imports the library.

A plain case is an episode case of tests/amppi_episode_cases.py plus its `rules` (the keys tests/svmpc_sim_cases.py reads), so that the
float64 restatement (`amppi_cases._step`, `_costs`, `_collisions`), the fp32 predicate replicas (`svmpc_sim_cases.crashed32`, `goal32`,
`apply_rules`) and the plant tolerance serve here unchanged - imported, never copied.

Forced events.  The device's actions are not known in advance, so events are forced by the start state and proven by `forced_events`
from the float64 step alone, under the TRUE rows, at every corner of the action box (and its centre) in every period up to the event,
with svmpc_sim_cases' MARGIN_CELLS / MARGIN_S to spare:
  part_map  0: starts ON an occupied cell - the plant's collision freeze holds it there: crash in period 0;
            1: starts inside the goal radius at low speed: goal in period 0;
            2: starts one period short of the block at x = -3.1 with 4 m/s toward it - a position moves by the OLD velocity, which one
               period's bounded acceleration changes by at most 0.15 m/s: crash in period 1 whatever the actions;
            3: reaches neither within T.
  skid_nav  0: every corner of the wheel-speed box puts it on an occupied cell of the navigation map in period 0;
            1: sits in the middle of 3 x 3 free blocks, further from every occupied cell than T periods at full speed.

`cost_tolerance(case)` follows svmpc_sim_cases.measure on this table: from the float64 restatement alone - never from device output.
"""
import itertools

import numpy as np

import amppi_cases as ac
import amppi_episode_cases as aec
import svmpc_episode_cases as sec
import svmpc_sim_cases as sc
from helpers import elemerr

TOL_FLOOR, TOL_CAP = sc.TOL_FLOOR, sc.TOL_CAP
MARGIN_CELLS, MARGIN_S = sc.MARGIN_CELLS, sc.MARGIN_S
COST_POWER = 5.0  # the least distance, in cost tolerances, a recorded cost keeps from each wrong cost in at least one period
NO_RULES = sc.NO_RULES
PART_GOAL = sc.PART_GOAL

costs64, crashed32, goal32, apply_rules, grid_of, cell_of = sc.costs64, sc.crashed32, sc.goal32, sc.apply_rules, sc.grid_of, sc.cell_of
crashed64, goal_s64, cost_variants, variant_distance = sc.crashed64, sc.goal_s64, sc.cost_variants, sc.variant_distance
family, start_states, start_sequences, plant_rows, plant_step, tick_params, context_kwargs, param_rows = (
    aec.family, aec.start_states, aec.start_sequences, aec.plant_rows, aec.plant_step, aec.tick_params, aec.context_kwargs, aec.param_rows)


def _case(tag, family, S, H, mode, up, T, B, seed, rules, **kw):
    return dict(aec._case(tag, family, S, H, mode, up, T, B, seed, **kw), rules=dict(NO_RULES, **rules))


REL4 = ((1.4,), (0.7,), (1.2,), (0.85,))
CASES = [
    # the first S with a second workgroup per environment; cost only
    _case("pend257", "pendulum", 257, 8, "extended", ("length", "mass"), 3, 3, 3101, {}, true_rel=aec.REL2),
    # the four events on Particle's own map
    _case("part_map", "particle", 256, 10, "extended", ("mass",), 3, 4, 3102, dict(goal=PART_GOAL, radius=1.0, crash=True), true_rel=REL4,
          start=((-2.03, -6.04, 1.0, -2.0), (8.8, 8.9, 0.1, -0.1), (-3.19, -6.03, 4.0, 0.0), (4.4, 0.3, -3.0, 4.5))),
    # the navigation cost's map in LDS, and a crash on it
    _case("skid_nav", "skid", 63, 8, "single", ("x_icr",), 2, 2, 3103, dict(crash=True), true_rel=((1.4,), (0.6,)), nav=True,
          start=((-0.53021691, -0.54962596, -0.82679324, 0.1, 0.0), (-0.66, 0.10, 0.4, 0.1, -0.05))),
    # a ragged last workgroup, one shared row per environment, the goal rule alone
    _case("cart1021", "cartpole", 1021, 8, "single", ("mass_pole", "length"), 3, 2, 3104, dict(goal=ac.CART["goal"], radius=0.3),
          true_rel=((1.4, 0.6), (0.6, 1.4))),
    _case("pend_ut", "pendulum", 64, 8, "ut", ("length",), 3, 2, 3105, dict(goal=(0.0, 0.0), radius=0.5), true_rel=aec.REL1),
    _case("roll3", "pendulum", 64, 8, "none", (), 3, 2, 3106, {}, roll_steps=3),
    _case("one", "pendulum", 1, 1, "none", (), 1, 1, 3107, {}, start=((1.5, 3.0),)),
]
BY_ID = {c["id"]: c for c in CASES}
IDS = [c["id"] for c in CASES]

# {case: {environment: (period, status)}}; an environment of these cases that is absent reaches neither event within T
EVENTS = {"part_map": {0: (0, 2), 1: (0, 1), 2: (1, 2)}, "skid_nav": {0: (0, 2)}}

# The dual cases (tests/test_gpu_amppi_dual_sim.py builds them through the pairs of tests/test_gpu_amppi_dual_batch.py, B = 3):
# family, mode, S, H, Mp, fixed bandwidth or None (Silverman), with actions_prev, rules, start states or None (the pairs' own)
DUAL = [
    dict(id="pend_ext", family="pendulum", mode="extended", S=257, H=12, Mp=65, bw=None, first=True, T=3,
         rules=dict(NO_RULES, goal=(0.0, 0.0), radius=0.5), start=None),
    # environment 0 starts on an occupied cell (crash in period 0), environment 2 one period short of the block (crash in period 1)
    dict(id="part_mass", family="particle", mode="single", S=64, H=10, Mp=3, bw=0.05, first=True, T=3,
         rules=dict(NO_RULES, goal=PART_GOAL, radius=1.0, crash=True),
         start=((-2.03, -6.04, 1.0, -2.0), (4.4, 0.3, -3.0, 4.5), (-3.19, -6.03, 4.0, 0.0))),
    dict(id="pend_sigma", family="pendulum", mode="sigma", S=64, H=8, Mp=1, bw=0.05, first=False, T=3,
         rules=dict(NO_RULES), start=None),
]
DUAL_BY_ID = {c["id"]: c for c in DUAL}
DUAL_EVENTS = {"part_mass": {0: (0, 2), 2: (1, 2)}}


DUAL_REL = (1.25, 0.8, 1.15)  # the true rows of the dual cases: the filters' mean particle times this, per environment
DUAL_UP = dict(pendulum=("length", "mass"), particle=("mass",))


def dual_as_case(d):
    """the dual case as a case of this table's kind - the float64 restatement, the rules' replicas, the tolerances and `shows` read it -
    under the id "dual_<id>" (in BY_ID, not among the IDS: the plain GPU tests do not run it)"""
    return BY_ID["dual_" + d["id"]]


for _d in DUAL:
    _up = DUAL_UP[_d["family"]]
    _c = _case("dual_" + _d["id"], _d["family"], _d["S"], _d["H"], dict(extended="extended", single="single", sigma="ut")[_d["mode"]], _up, _d["T"], 3,
               3200 + len(BY_ID), {k: v for k, v in _d["rules"].items() if k in ("goal", "radius", "crash")}, start=_d["start"],
               true_rel=tuple((r,) * len(_up) for r in DUAL_REL))
    BY_ID[_c["id"]] = _c
    if _d["id"] in DUAL_EVENTS:
        EVENTS[_c["id"]] = DUAL_EVENTS[_d["id"]]


# ------------------------------------------------------------------------------------------------ forced events
def _frac_margin(grid, xy, cell):
    return sc._frac_margin(grid, xy, cell)


def _corners(f):
    lo, hi = np.asarray(f["lo"], np.float64), np.asarray(f["hi"], np.float64)
    axes = [(lo[k], hi[k], 0.0) for k in range(len(lo))]
    return np.array(list(itertools.product(*axes)), np.float64)


def _reach(case, b, rows):
    """the furthest a position moves in one period"""
    f = family(case)
    if case["family"] == "particle":
        return f["max_speed"] * f["dt"]
    d = dict(f["defaults"])
    if rows is not None:
        d.update({k: float(rows[b, i]) for i, k in enumerate(case["up"])})
    top = max(abs(v) for v in tuple(f["lo"]) + tuple(f["hi"]))
    lin = 2 * top * np.pi * d["wheel_radius"] * f["dt"]
    lat = 2 * top * 2 * np.pi * d["wheel_radius"] / d["axial_distance"] * abs(d["x_icr"]) * f["dt"]
    return float(np.hypot(lin, lat))


def forced_events(case, grid, events=None, start=None, rows="case"):
    """Proves the events of a case from the float64 step alone, under the true rows and at every corner of the action box in every period
    up to the event; -> {environment: (least margin in cells or None, least margin in s or None)}.  The reachable set of a period is not
    convex in general; the corners stand for it where the step is affine in the clamped action (Particle) and bound it by `_reach`
    where an environment must NOT meet an event."""
    f, r = family(case), case["rules"]
    events = EVENTS.get(case["id"], {}) if events is None else events
    x0 = (start_states(case) if start is None else np.asarray(start, np.float32)).astype(np.float64)
    rows = plant_rows(case) if isinstance(rows, str) else rows
    cell, corners = cell_of(case), _corners(f)
    nx, ny = grid.shape
    centre = np.array([int(nx / 2), int(ny / 2)])
    out = {}
    for b in range(len(x0)):
        ev = events.get(b)
        x = x0[b:b + 1]
        if ev is None:
            reach = _reach(case, b, rows) * case["T"]
            assert not crashed64(case, x, grid)[0]
            lo = np.floor((x[0, :2] - reach) / cell + centre).astype(int)
            hi = np.floor((x[0, :2] + reach) / cell + centre).astype(int)
            assert not grid[max(lo[0], 0):hi[0] + 1, max(lo[1], 0):hi[1] + 1].any(), "an occupied cell within reach"
            if r["goal"] is not None:
                dist = np.linalg.norm(np.asarray(r["goal"], np.float64)[:2] - x[0, :2]) - reach
                assert dist > 0 and dist * dist > r["radius"] ** 2 + MARGIN_S
            out[b] = (None, None)
            continue
        period, status = ev
        row = None if rows is None else rows[b:b + 1]
        nxt = x
        for t in range(period + 1):
            if t:  # no event before the forced one, at any corner so far
                assert not crashed64(case, nxt, grid).any() and _frac_margin(grid, nxt[:, :2], cell) >= MARGIN_CELLS
                assert r["goal"] is None or goal_s64(case, nxt).min() > r["radius"] ** 2 + MARGIN_S
            n = len(nxt)
            xs = np.repeat(nxt, len(corners), 0)
            acts = np.tile(corners, (n, 1)) * 3.0  # (x 3: beyond the clamp, onto it)
            nxt = plant_step(case, xs, acts, None if row is None else np.repeat(row, len(xs), 0), grid if case["family"] == "particle" else None)
        if status == 2:
            assert crashed64(case, nxt, grid).all()
            out[b] = (_frac_margin(grid, nxt[:, :2], cell), None)
            assert out[b][0] >= MARGIN_CELLS
        else:
            assert not crashed64(case, nxt, grid).any() and _frac_margin(grid, nxt[:, :2], cell) >= MARGIN_CELLS
            out[b] = (None, float(r["radius"] ** 2 - goal_s64(case, nxt).max()))
            assert out[b][1] >= MARGIN_S
    return out


# ------------------------------------------------------------------------------------------------ the cost check's tolerance and power
_measured = {}


def measure(cid):
    """(d, tol, {variant: distance in tolerances}) of a plain case from the restatement alone: svmpc_sim_cases.measure on this table"""
    if cid in _measured:
        return _measured[cid]
    case = BY_ID[cid]
    grid = grid_of(case)
    xs, _, _ = aec.restated_loop(case, grid if case["family"] == "particle" else None)  # [T + 1, B, ds] fp32
    T = case["T"]
    exact = np.stack([costs64(case, xs[t + 1].astype(np.float64), grid) for t in range(T)])
    f32 = np.stack([costs64(case, xs[t + 1], grid) for t in range(T)])
    moved = np.stack([costs64(case, sec.ulp_moved(xs[t + 1], case["seed"] + t).astype(np.float64), grid) for t in range(T)])
    d = max(elemerr(f32, exact), elemerr(moved, exact))
    tol = max(TOL_FLOOR, 2.0 * d)
    var = {}
    for t in range(T):
        for k, v in cost_variants(case, xs[t].astype(np.float64), xs[t + 1].astype(np.float64), grid).items():
            var.setdefault(k, []).append(v)
    power = {k: variant_distance(exact, np.stack(v), tol) for k, v in var.items()}
    _measured[cid] = (d, tol, power)
    return _measured[cid]


def cost_tolerance(case):
    d, tol, _ = measure(case["id"])
    assert tol <= TOL_CAP, (case["id"], d)
    return tol


def shows(case, variant):
    """whether a case can show a wrong cost: the obstacle term only where a recorded state lies on an occupied cell (a forced crash)"""
    if variant == "no_obstacle":
        return any(st == 2 for _, st in EVENTS.get(case["id"], {}).values())
    return True


def plant_tolerance(case):
    """amppi_episode_cases.measure's tolerance on a case of this table: from the restatement alone"""
    grid = grid_of(case) if case["family"] == "particle" else None
    xs, acts, exact = aec.restated_loop(case, grid)
    rows = plant_rows(case)
    T = acts.shape[0]
    f32 = np.stack([plant_step(case, xs[t], acts[t], rows, grid, dtype=np.float32) for t in range(T)])
    moved = np.stack([plant_step(case, sec.ulp_moved(xs[t], case["seed"] + t), acts[t], rows, grid) for t in range(T)])
    tol = max(TOL_FLOOR, 2.0 * max(elemerr(f32, exact), elemerr(moved, exact)))
    assert tol <= TOL_CAP, (case["id"], tol)
    return tol


def loss32(costs, n):
    """the sequential float32 sum of the first n costs"""
    s = np.float32(0.0)
    for t in range(n):
        s = np.float32(s + np.float32(costs[t]))
    return s
