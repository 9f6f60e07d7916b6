"""Cases (TEST INFRASTRUCTURE) for dust_svmpc_dual_batch_simulate and dust_svmpc_dual_batch_optimize - the DuSt-MPC episode under the
reference's rules: warm-up with the filters updating, the accumulated cost, crash and goal -, shared by
tests/test_svmpc_dual_sim_cpu.py and tests/test_gpu_svmpc_dual_sim.py.  Data and seeded numpy only: nothing here imports the library.

A case is a dual-episode case (tests/svmpc_dual_episode_cases.py `_case`: an episode case plus the filter side) plus its `rules`, in the
format of tests/svmpc_sim_cases.py, so that the float64 restatements (`svmpc_episode_cases.plant_step`, `svmpc_sim_cases.costs64`,
`crashed64`, `goal_s64`), the fp32 replicas (`crashed32`, `goal32`, `apply_rules`) and the tolerances (`plant_tolerance`,
`cost_tolerance`) are imported and never copied.  The TRUE parameter rows differ from the nominal ones by 10 - 40 %, another factor per
environment.

Forced events.  The device's actions are not known in advance, so the Particle cases force their events by the start state, under the
TRUE rows.  `part_events` (no warm-up): environment 0 starts ON an occupied cell - the plant's collision freeze holds it there, so its
new position is occupied whatever the action -, environment 1 starts inside the goal radius and stays inside for every action within
the clamps (the position moves by the OLD velocity; the velocity by at most max_accel dt per axis; s is convex, so the corners of the
clamp box bound it).  `part_warm_events` (warm_up 3): the zero action makes the first three steps exact - a crash in period 1, a goal in
period 1, a goal in period 2, one environment that runs on into the tick.  `forced_events` proves all of it from the float64 step with
svmpc_sim_cases' MARGIN_CELLS and MARGIN_S to spare.
"""
import numpy as np

import svmpc_dual_episode_cases as dec
import svmpc_episode_cases as ec
import svmpc_sim_cases as sc

FACTOR = dec.FACTOR  # the plant keeps the dual-episode cases' distance from its three wrong plants
COST_FACTOR = 5.0    # ... and at least one recorded cost this many tolerances from each wrong cost the case can show
PART_GOAL = sc.PART_GOAL


def _case(tag, *args, rules=None, **kw):
    return dict(dec._case(tag, *args, **kw), rules=dict(sc.NO_RULES, **(rules or {})))


_PART = dict(kernel="K1", optimizer="SGD", lr=100.0, sigma_p=5.0, roll_strategy="mean", weighted_prior=True)
_SGD = dict(kernel="K1", optimizer="SGD", lr=2.0, sigma_p=2.0)
CASES = [
    # the common path under warm-up: two periods without forward() whose filters update, then three ticks
    _case("pend_warm", "pendulum", 3, 8, 3, 5, 1, 5, 3, ("length", "mass"), 3101, _SGD, 1.0, ((1.25, 0.8), (0.8, 1.2), (1.15, 1.3)), 48, 3, None, "SGD",
          start=dec.PEND_START, rules=dict(warm_up=2)),
    # Adam reads t0; Mp = 65 leaves the padded width; n_steps > 1; the call hands actions_prev: the warm-up period 0 updates too
    _case("pend_adam_first", "pendulum", 4, 16, 8, 6, 3, 4, 2, ("g", "mass", "length"), 3102, dict(kernel="IMQ", optimizer="Adam", lr=0.5, sigma_p=2.0),
          1.0, ((0.85, 1.3, 0.75), (1.2, 0.7, 1.35)), 65, 2, 0.3, "Adam", first=True, start=dec.PEND_START, rules=dict(warm_up=1)),
    # log space on both sides, three filter particles, no warm-up; the goal rule is on but out of reach (the pendulum falls from 3 rad)
    _case("pend_log", "pendulum", 2, 4, 1, 3, 2, 3, 2, ("length",), 3103, _SGD, 1.0, ((1.3,), (0.7,)), 3, 2, None, "SGD", log=True, start=dec.PEND_START,
          rules=dict(goal=(0.0, 0.0), radius=0.5)),
    # events in period 0 whatever the controller picks: 0 crashes (it starts on an occupied cell), 1 is inside the radius, 2 and 3 run on
    _case("part_events", "particle", 3, 8, 4, 4, 1, 3, 4, ("mass",), 3104, _PART, 3.0, ((1.3,), (0.75,), (0.85,), (1.15,)), 48, 2, 0.5, "SGD",
          start=((-2.03, -6.04, 1.0, -2.0), (8.8, 8.9, 0.1, -0.1), (4.4, 0.3, -3.0, 4.5), (6.03, -8.04, -2.0, 1.0)),
          rules=dict(goal=PART_GOAL, radius=1.0, crash=True)),
    # events under the zero action: 0 crashes in period 1, 1 enters the radius in period 1, 2 in period 2, 3 runs on into the tick:
    # neighbours stop in different periods, and their filters stop with them
    _case("part_warm_events", "particle", 3, 8, 4, 4, 1, 4, 4, ("mass",), 3105, _PART, 3.0, ((1.3,), (0.75,), (0.85,), (1.15,)), 48, 2, None, "SGD",
          start=((-3.19, -6.03, 4.0, 0.0), (8.1225, 9.03, 0.5, 0.0), (8.115, 9.03, 0.5, 0.0), (4.4, 0.3, -3.0, 4.5)),
          rules=dict(warm_up=3, goal=PART_GOAL, radius=1.0, crash=True)),
    # every loop bound at 1; T = 1 without actions_prev: no filter launch at all.  Run with warm_up 0 and with warm_up 1 (WARM_TOO)
    _case("ones", "pendulum", 1, 1, 1, 1, 1, 1, 1, ("length",), 3106, _SGD, 1.0, ((1.3,),), 1, 1, 0.1, "SGD", start=dec.PEND_START),
]
BY_ID = {c["id"]: c for c in CASES}
IDS = [c["id"] for c in CASES]
WARM_TOO = {"ones": 1}  # the case also runs under this warm_up: no forward() at all, a_seq and pw_out stay unwritten

# {case: {environment: (period, status)}}; an environment that is absent reaches neither event within T
EVENTS = {"part_events": {0: (0, 2), 1: (0, 1)}, "part_warm_events": {0: (1, 2), 1: (1, 1), 2: (2, 1)}}


def with_rules(case, **rules):
    """the case under other rules (with_rules(case, **svmpc_sim_cases.NO_RULES): the plain dual episode)"""
    return dict(case, rules=dict(case["rules"], **rules))


def grid_of(case):
    return sc.grid_of(case)


def cost_case(case):
    """the case of tests/svmpc_sim_cases.py whose measured cost tolerance holds for this family"""
    return sc.BY_ID["pend" if case["family"] == "pendulum" else "part"]


def cost_tolerance(case):
    return sc.cost_tolerance(cost_case(case))


def expected(case):
    """(n_run [B], status [B]) the forced events give; environments without an event run the T periods"""
    n, st = np.full(case["B"], case["T"], np.int32), np.zeros(case["B"], np.int32)
    for b, (period, status) in EVENTS.get(case["id"], {}).items():
        n[b], st[b] = period + 1, status
    return n, st


# ------------------------------------------------------------------------------------------------ forced events, under the TRUE rows
def forced_events(case, grid):
    """Proves EVENTS[case] from the float64 step under the true rows; -> {environment: (margin in cells or None, margin in s or None)}"""
    f, r = ec.family(case), case["rules"]
    x0 = ec.start_states(case).astype(np.float64)
    rows = dec.true_rows(case).astype(np.float64)
    amax, vmax, dt, cell = f["max_accel"], f["max_speed"], f["dt"], f["cell"]
    out = {}
    for b in range(case["B"]):
        ev = EVENTS[case["id"]].get(b)
        x, row = x0[b:b + 1], rows[b:b + 1]
        if ev is None:  # within T periods at max_speed it reaches no occupied cell and stays outside the radius
            assert not sc.crashed64(case, x, grid)[0]
            reach = vmax * dt * case["T"]
            nx, ny = grid.shape
            half = np.array([int(nx / 2), int(ny / 2)])
            lo = np.floor((x[0, :2] - reach) / cell + half).astype(int)
            hi = np.floor((x[0, :2] + reach) / cell + half).astype(int)
            assert lo.min() >= 1 and not grid[lo[0] - 1:hi[0] + 2, lo[1] - 1:hi[1] + 2].any(), "an occupied cell within reach"
            dist = np.linalg.norm(np.asarray(r["goal"], np.float64)[:2] - x[0, :2]) - reach
            assert dist > 0 and dist * dist > r["radius"] ** 2 + sc.MARGIN_S
            out[b] = (None, None)
            continue
        period, status = ev
        if r["warm_up"] == 0:  # every action inside the clamps: the corners of the clamp box (and its centre), pushed beyond it
            assert period == 0
            m = float(row[0, 0])
            corners = np.array([[sx * amax * m, sy * amax * m] for sx in (-1, 1) for sy in (-1, 1)] + [[0.0, 0.0]], np.float64) * 3.0
            nxt = ec.plant_step(case, np.repeat(x, len(corners), 0), corners, np.repeat(row, len(corners), 0), grid)
        else:  # the zero action: the steps up to the event are exact, and no earlier period shows an event
            assert period < r["warm_up"]
            nxt = x
            for t in range(period + 1):
                assert not sc.crashed64(case, nxt, grid)[0] and sc._frac_margin(grid, nxt[:, :2], cell) >= sc.MARGIN_CELLS
                if t:
                    assert sc.goal_s64(case, nxt)[0] > r["radius"] ** 2 + sc.MARGIN_S
                nxt = ec.plant_step(case, nxt, np.zeros((1, 2)), row, grid)
        s = sc.goal_s64(case, nxt)
        if status == 2:
            assert sc.crashed64(case, nxt, grid).all()
            out[b] = (sc._frac_margin(grid, nxt[:, :2], cell), None)
            assert out[b][0] >= sc.MARGIN_CELLS
        else:
            assert not sc.crashed64(case, nxt, grid).any() and sc._frac_margin(grid, nxt[:, :2], cell) >= sc.MARGIN_CELLS
            out[b] = (None, float(r["radius"] ** 2 - s.max()))
            assert out[b][1] >= sc.MARGIN_S
        # the fp32 replicas agree with the float64 predicates at those states
        x32 = nxt.astype(np.float32)
        assert np.array_equal(sc.crashed32(grid, x32[:, :2], cell), sc.crashed64(case, nxt, grid))
        assert np.array_equal(sc.goal32(r["goal"], r["radius"], x32), s <= r["radius"] ** 2)
    return out


# ------------------------------------------------------------------------------------------------ the loop, restated
def restated_loop(case, grid=None):
    """The float64 closed loop of the case under its true rows, its rules and svmpc_dual_episode_cases' stand-in controller (the zero
    action while the episode warms up; a stopped environment keeps its last state): (states [T + 1, B, ds] fp32 as the device carries
    them, actions [T, B, da] fp32, exact float64 steps [T, B, ds], n_run [B], status [B])"""
    rows, r = dec.true_rows(case), case["rules"]
    B, T = case["B"], case["T"]
    xs, acts, exact = [ec.start_states(case)], [], []
    n_run, status = np.zeros(B, np.int32), np.zeros(B, np.int32)
    for t in range(T):
        a = dec.stand_in_actions(case, xs[-1], t)
        if t < r["warm_up"]:
            a = np.zeros_like(a)
        step = ec.plant_step(case, xs[-1], a, rows, grid)
        on = status == 0
        step[~on] = xs[-1][~on]
        acts.append(a)
        exact.append(step)
        xs.append(step.astype(np.float32))
        n_run[on] += 1
        status[on] = sc.apply_rules(case, xs[-1], grid)[on]
    return np.stack(xs), np.stack(acts), np.stack(exact), n_run, status


def cost_power(case, xs, n_run, grid, tol, costs=None):
    """{variant: the largest distance, in tolerances, over the periods each environment ran, of the costs (default: the float64 cost of
    xs[t + 1]) from that wrong cost on the same states}: the previous state's cost, the terminal weights (the Pendulum's two costs are
    one function), the cost without its obstacle term (a case shows it only when a recorded state lies on an occupied cell)"""
    far = {}
    for t in range(len(xs) - 1):
        on = n_run > t
        if not on.any():
            continue
        new = xs[t + 1][on].astype(np.float64)
        got = sc.costs64(case, new, grid) if costs is None else np.asarray(costs[t], np.float64)[on]
        for k, v in sc.cost_variants(case, xs[t][on].astype(np.float64), new, grid).items():
            far[k] = max(far.get(k, 0.0), sc.variant_distance(got, v, tol))
    return far


def cost_variants_shown(case):
    """the wrong costs the case can show (see cost_power)"""
    if case["family"] == "pendulum":
        return {"prev_state"}
    return {"prev_state", "terminal", "no_obstacle"} if case["id"] in EVENTS else {"prev_state", "terminal"}
