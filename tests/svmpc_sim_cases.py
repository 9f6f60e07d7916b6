"""Cases (TEST INFRASTRUCTURE) for dust_svmpc_batch_simulate - the closed-loop episode under the reference's rules: warm-up, the
accumulated cost, crash and goal -, shared by tests/test_svmpc_sim_cpu.py and tests/test_gpu_svmpc_sim.py.  Data and seeded numpy only:
nothing here imports the library.

A case is an episode case of tests/svmpc_episode_cases.py (itself an AMPPI scenario dict, tests/amppi_cases.py `A`) plus its `rules`, so
that the float64 restatement - `amppi_cases._step`, `_costs`, `_collisions` - is imported and never copied.

Forced events.  The device's actions are not known in advance, so the Particle cases force their events by the start state: an
environment that every admissible acceleration crashes in period 0, one that every admissible acceleration keeps inside the goal radius
after period 0, one that can reach neither within T, and - under warm-up, where the action is zero and the step therefore exact - events
in period 1.  `forced_events` proves these from the float64 step alone, with MARGIN_CELLS and MARGIN_S to spare.

`cost_tolerance(case)` follows `svmpc_episode_cases.plant_tolerance`: measured from the restatement alone on a float64 closed loop of the
case's own start states, true rows and seeded actions - never from device output -, d = max(elemerr(cost on float32 operands, float64
cost), elemerr(cost of states moved one fp32 ulp, float64 cost)), tol = max(1e-5, 2 d), capped at 5e-5.  `COST_POWER` is the least
distance, in tolerances, that at least one recorded cost must keep from each wrong variant a case can show.
"""
import numpy as np

import amppi_cases as ac
import svmpc_episode_cases as ec
from helpers import elemerr

TOL_FLOOR, TOL_CAP = ec.TOL_FLOOR, ec.TOL_CAP
MARGIN_CELLS, MARGIN_S = 1e-3, 1e-3  # what a forced event keeps from a cell edge (in cells) and from r^2 (in s)
NO_RULES = dict(warm_up=0, goal=None, radius=None, crash=False)
PART_GOAL = ac.PART["target"]


def _case(tag, family, N, S, M, H, n_steps, T, B, up, seed, opts, scale, rules, rows=False, **kw):
    return dict(ec._case(tag, family, N, S, M, H, n_steps, T, B, up, seed, opts, scale, **kw), rules=dict(NO_RULES, **rules), rows=rows)


_PEND = dict(kernel="K1", optimizer="SGD", lr=2.0, sigma_p=2.0)
_PART = dict(kernel="K1", optimizer="Adam", lr=1.0, sigma_p=5.0, roll_strategy="mean", weighted_prior=True)
_SKID = dict(kernel="IMQ", optimizer="SGD", lr=0.05, sigma_p=0.3)
CASES = [
    # SGD / K1, warm_up = 2 < T; the goal rule is on but out of reach
    _case("pend", "pendulum", 3, 16, 3, 6, 2, 4, 3, ("length", "mass"), 2101, _PEND, 1.0, dict(warm_up=2, goal=(0.0, 0.0), radius=0.5),
          true_rel=((1.25, 0.8), (0.8, 1.2), (1.15, 1.3))),
    # Adam / roll "mean" on the demo's map, no warm-up: environment 0 crashes in period 0 (just left of the block at x = -3.1 .. -0.9,
    # heading into it), environment 1 sits inside the goal radius, environment 2 can reach neither within T
    _case("part", "particle", 4, 16, 1, 5, 1, 3, 3, (), 2102, _PART, 3.0, dict(goal=PART_GOAL, radius=1.0, crash=True),
          start=((-3.15, -6.03, 4.0, 0.5), (8.8, 8.9, 0.1, -0.1), (4.4, 0.3, -3.0, 4.5))),
    # ... warm_up = 2: the zero action makes period 1 exact - environment 0 crashes in it, environment 1 enters the radius in it
    # (s = 1.0078 after period 0, 0.9948 after period 1), environment 2 runs on into the ticks
    _case("part_warm", "particle", 4, 16, 1, 5, 1, 4, 3, (), 2103, _PART, 3.0, dict(warm_up=2, goal=PART_GOAL, radius=1.0, crash=True),
          start=((-3.19, -6.03, 4.0, 0.0), (8.1225, 9.03, 0.5, 0.0), (4.4, 0.3, -3.0, 4.5))),
    _case("skid_nav", "skid", 4, 16, 2, 6, 1, 3, 2, ("x_icr",), 2104, _SKID, 0.3, dict(warm_up=1, goal=ac.SKID["goal"], radius=0.05, crash=True),
          true_rel=((1.5,), (0.6,)), nav=True, start=((0.307, -0.193, 0.4, 0.1, -0.05), (0.357, -0.093, 0.55, 0.3, 0.2))),  # (off the cell edges)
    _case("cart", "cartpole", 2, 16, 2, 5, 1, 3, 2, ("mass_pole", "length"), 2105, dict(kernel="K1", optimizer="SGD", lr=0.05, sigma_p=0.5), 0.5,
          dict(warm_up=1, goal=ac.CART["goal"], radius=0.1), true_rel=((2.0, 0.6), (0.5, 1.5))),
    _case("one", "pendulum", 1, 1, 1, 1, 1, 1, 1, (), 2106, _PEND, 1.0, dict(warm_up=1), start=((1.5, 3.0),)),
    # per-environment hyper-parameter rows (hyper_rows): the sweep instances
    _case("pend_rows", "pendulum", 3, 16, 3, 6, 2, 3, 4, ("length", "mass"), 2107, _PEND, 1.0, dict(warm_up=1, goal=(0.0, 0.0), radius=0.5),
          rows=True, true_rel=((1.25, 0.8), (0.8, 1.2), (1.15, 1.3), (0.9, 0.9))),
]
BY_ID = {c["id"]: c for c in CASES}
IDS = [c["id"] for c in CASES]

# What the Particle cases force: {case: {environment: (period, status)}}; an environment that is absent reaches neither event within T
EVENTS = {"part": {0: (0, 2), 1: (0, 1)}, "part_warm": {0: (1, 2), 1: (1, 1)}}

# Least distance, in cost tolerances, that at least one recorded cost keeps from each wrong variant the case can show: the cost of the
# state BEFORE the step, the terminal weights in place of the instantaneous ones (the Pendulum's two costs are one function), the cost
# without its obstacle term (a case shows it only when a recorded state lies on an occupied cell: `part` and `part_warm` by their forced
# crash).  tests/test_svmpc_sim_cpu.py asserts ten times these floors on the float64 restatement of the seeded loops.
COST_POWER = {
    "pend": dict(prev_state=5.0),
    "part": dict(prev_state=5.0, terminal=5.0, no_obstacle=5.0),
    "part_warm": dict(prev_state=5.0, terminal=5.0, no_obstacle=5.0),
    "skid_nav": dict(prev_state=5.0, terminal=5.0, no_obstacle=5.0),
    "cart": dict(prev_state=5.0, terminal=5.0),
    "one": dict(prev_state=5.0),
    "pend_rows": dict(prev_state=5.0),
}


def grid_of(case):
    """the occupancy map of the case (Particle: the demo's grid_4x4; the navigation cost: svmpc_episode_cases.nav_map) or None"""
    if case["family"] == "particle":
        from oracle import grid_4x4_map

        return grid_4x4_map()
    return ec.nav_map() if case["nav"] else None


def cell_of(case):
    return ac.PART["cell"] if case["family"] == "particle" else ec.NAV["cell_size"]


def hyper_rows(base, B):
    """[B] rows from the prototype's own (`base`: SvmpcBatch.get_hyper() of the batch): 0 the prototype's values, 1 lr x 4, 2 alpha x 2 and
    temperature / 2 (the product stays: the one-softmax path), 3 alpha x 2 alone (the two-softmax path beside it), a narrower prior and
    the weighted mixture"""
    rows = {k: np.array(v) for k, v in base.items()}
    rows["lr"][1] *= 4.0
    rows["alpha"][2] *= np.float32(2.0)
    rows["temperature"][2] *= np.float32(0.5)
    rows["alpha"][3] *= np.float32(2.0)
    rows["sigma_p"][3] *= np.float32(0.5)
    rows["weighted_prior"][3] = 1
    assert B == 4
    return rows


def row_kwargs(rows, b):
    """the Context keywords that build a prototype with row b's values (the action covariance is not varied: it stays the case's a_cov)"""
    return dict(lr=float(rows["lr"][b]), alpha=float(rows["alpha"][b]), temperature=float(rows["temperature"][b]),
                sigma_p=np.asarray(rows["sigma_p"][b], np.float32), weighted_prior=bool(rows["weighted_prior"][b]))


# ------------------------------------------------------------------------------------------------ the rules, restated
def costs64(case, x, grid, term=False, obstacle=True):
    """controller.inst_cost_fn of states x [n, ds] in float64: amppi_cases._costs, under the navigation cost plus w_obs x collision"""
    x = np.asarray(x)
    if case["family"] == "particle" and not obstacle:
        grid = np.zeros_like(grid)
    c = ac._costs(case, x, grid, term)
    if case["nav"] and obstacle:
        c = c + ec.NAV["w_obs"] * ac._collisions(grid, np.asarray(x[:, :2], np.float64), cell_of(case))
    return c


def crashed64(case, x, grid):
    return ac._collisions(grid, np.asarray(x, np.float64)[:, :2], cell_of(case)) != 0


def goal_s64(case, x):
    d = np.asarray(case["rules"]["goal"], np.float64) - np.asarray(x, np.float64)
    return (d * d).sum(-1)


def crashed32(grid, xy, cell):
    """the device's lookup (common.hpp collision) in fp32 numpy, operation for operation: floor(x * (float)(1 / cell) + offset), clamped"""
    nx, ny = grid.shape
    xy = np.asarray(xy, np.float32)
    inv = np.float32(1.0 / cell)
    fx = np.floor(xy[:, 0] * inv + np.float32(int(nx / 2)))
    fy = np.floor(xy[:, 1] * inv + np.float32(int(ny / 2)))
    ix = np.where(fx >= 0, np.minimum(fx, np.float32(nx - 1)), np.float32(0)).astype(np.int64)
    iy = np.where(fy >= 0, np.minimum(fy, np.float32(ny - 1)), np.float32(0)).astype(np.int64)
    return grid[ix, iy] != 0


def goal32(goal, radius, x):
    """the device's goal rule in fp32 numpy: d_k = goal_k - x_k, s = ((d_0 d_0 + d_1 d_1) + d_2 d_2) + .., s <= (float)(radius * radius)"""
    x, g = np.asarray(x, np.float32), np.asarray(goal, np.float32)
    s = None
    for k in range(x.shape[-1]):
        d = g[k] - x[:, k]
        s = d * d if s is None else s + d * d
    return s <= np.float32(float(radius) * float(radius))


def apply_rules(case, x, grid):
    """status [n] int32 of states x [n, ds] (fp32, as the device recorded them) by the fp32 replicas: 2 crash (wins), 1 goal, 0 neither"""
    r = case["rules"]
    st = np.zeros(len(x), np.int32)
    if r["goal"] is not None:
        st[goal32(r["goal"], r["radius"], x)] = 1
    if r["crash"]:
        st[crashed32(grid, x[:, :2], cell_of(case))] = 2
    return st


# ------------------------------------------------------------------------------------------------ forced events
def _frac_margin(grid, xy, cell):
    """least distance, in cells, of the positions xy [n, 2] (float64) from a cell edge"""
    nx, ny = grid.shape
    c = xy * (1 / cell) + np.array([int(nx / 2), int(ny / 2)], np.float64)
    f = c - np.floor(c)
    return float(np.minimum(f, 1 - f).min())


def forced_events(case, grid):
    """Proves EVENTS[case] from the float64 step alone; -> {environment: (least margin in cells or None, least margin in s or None)}.
    Period 0 without warm-up: the step is affine in the clamped acceleration, so the corners of the clamp box bound the reachable state;
    s is convex, so its maximum over the box lies at a corner.  Under warm-up the action is zero and the two steps are exact.  An
    environment without an event: within T periods at max_speed it reaches no occupied cell and stays outside the radius."""
    f, r = ec.family(case), case["rules"]
    x0 = ec.start_states(case).astype(np.float64)
    mass, amax, vmax, dt, cell = f["defaults"]["mass"], f["max_accel"], f["max_speed"], f["dt"], f["cell"]
    out = {}
    for b in range(case["B"]):
        ev = EVENTS[case["id"]].get(b)
        x = x0[b:b + 1]
        assert not crashed64(case, x, grid)[0], "an environment starts on a free cell"
        if ev is None:
            reach = vmax * dt * case["T"]
            nx, ny = grid.shape
            lo = np.floor((x[0, :2] - reach) / cell + np.array([int(nx / 2), int(ny / 2)])).astype(int)
            hi = np.floor((x[0, :2] + reach) / cell + np.array([int(nx / 2), int(ny / 2)])).astype(int)
            assert not grid[lo[0] - 1:hi[0] + 2, lo[1] - 1:hi[1] + 2].any(), "an occupied cell within reach"
            dist = np.linalg.norm(np.asarray(r["goal"], np.float64)[:2] - x[0, :2]) - reach
            assert dist > 0 and dist * dist > r["radius"] ** 2 + MARGIN_S
            out[b] = (None, None)
            continue
        period, status = ev
        if r["warm_up"] == 0:
            assert period == 0
            corners = np.array([[sx * amax * mass, sy * amax * mass] for sx in (-1, 1) for sy in (-1, 1)] + [[0.0, 0.0]], np.float64)
            nxt = ac._step(case, np.repeat(x, len(corners), 0), corners * 3.0, dict(f["defaults"]), grid)  # (x 3: beyond the clamp, onto it)
        else:
            assert period < r["warm_up"]
            nxt = x
            for t in range(period + 1):
                if t:
                    assert not crashed64(case, nxt, grid)[0] and _frac_margin(grid, nxt[:, :2], cell) >= MARGIN_CELLS
                    assert goal_s64(case, nxt)[0] > r["radius"] ** 2 + MARGIN_S
                nxt = ac._step(case, nxt, np.zeros((1, 2)), dict(f["defaults"]), grid)
        s = goal_s64(case, nxt)
        if status == 2:
            assert crashed64(case, nxt, grid).all()
            out[b] = (_frac_margin(grid, nxt[:, :2], cell), None)
            assert out[b][0] >= MARGIN_CELLS
        else:
            assert not crashed64(case, nxt, grid).any() and _frac_margin(grid, nxt[:, :2], cell) >= MARGIN_CELLS
            out[b] = (None, float(r["radius"] ** 2 - s.max()))
            assert out[b][1] >= MARGIN_S
    return out


# ------------------------------------------------------------------------------------------------ the cost check's tolerance and power
def cost_variants(case, x_prev, x_new, grid):
    """the wrong costs on the same states, in float64: {variant: [n]}"""
    out = dict(prev_state=costs64(case, x_prev, grid))
    if case["family"] != "pendulum":
        out["terminal"] = costs64(case, x_new, grid, term=True)
    if grid is not None:
        out["no_obstacle"] = costs64(case, x_new, grid, obstacle=False)
    return out


def variant_distance(costs, variant, tol):
    """the largest element-wise distance, in tolerances, of the costs from a variant's ('in at least one period')"""
    v = np.asarray(variant, np.float64)
    floor = float(np.sqrt(np.mean(v * v)))
    return float((np.abs(np.asarray(costs, np.float64) - v) / (np.abs(v) + floor + 1e-300)).max()) / tol


_measured = {}


def measure(cid):
    """(d, tol, {variant: distance in tolerances}) of a case from the restatement alone (svmpc_episode_cases.restated_loop: a float64
    closed loop from seeded actions, its states rounded to fp32 as the device carries them)"""
    if cid in _measured:
        return _measured[cid]
    case = BY_ID[cid]
    grid = grid_of(case)
    xs, _, _ = ec.restated_loop(case, grid)  # [T + 1, B, ds] fp32
    T = case["T"]
    exact = np.stack([costs64(case, xs[t + 1].astype(np.float64), grid) for t in range(T)])
    f32 = np.stack([costs64(case, xs[t + 1], grid) for t in range(T)])  # (the operands in fp32)
    moved = np.stack([costs64(case, ec.ulp_moved(xs[t + 1], case["seed"] + t).astype(np.float64), grid) for t in range(T)])
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
