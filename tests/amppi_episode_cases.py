"""Closed-loop AMPPI episode cases (TEST INFRASTRUCTURE) for dust_amppi_batch_episode, shared by tests/test_amppi_episode_cpu.py and
tests/test_gpu_amppi_episode.py.  Data and seeded numpy only: nothing here imports the library.

A case is an AMPPI scenario dict (tests/amppi_cases.py `A`) plus the periods T, the environments B, the roll, the true parameter rows
relative to the nominal ones and the options of the map - the keys tests/svmpc_episode_cases.py reads, so that its start states, true
rows, float64 plant step (`amppi_cases._step`, imported - never copied), wrong variants and restated loop serve here unchanged.

The plant tolerance follows svmpc_episode_cases.measure, from the float64 restatement alone - never from device output:
d = max(elemerr(step on float32 operands, float64 step), elemerr(step on states moved one fp32 ulp, float64 step)), tol = max(1e-5, 2 d),
capped at 5e-5.  POWER is the least distance, in tolerances, the GPU test demands between the device's states and each wrong plant the
case can show (nominal row in place of the true one, the previous period's action, no step); RESTATED_MARGIN is how many times that the
restated loop itself must show (the CPU test asserts it), so that the floor separates a wrong plant from rounding with room on both sides.
"""
import numpy as np

import amppi_cases as ac
import svmpc_episode_cases as sec
from helpers import elemerr

TOL_FLOOR, TOL_CAP = sec.TOL_FLOOR, sec.TOL_CAP
NAV = sec.NAV
POWER = 5.0
RESTATED_MARGIN = 4.0
FULL_COV = ac.BY_TAG["skid_none_63"]["a_cov"]


def _case(tag, family, S, H, mode, up, T, B, seed, true_rel=None, start=None, nav=False, roll_steps=1, map_dev=False, **kw):
    return dict(ac.A("amppi_episode_" + tag, family, S, H, mode, up, seed, **kw), id=tag, T=T, B=B, true_rel=true_rel, start=start, nav=nav,
                roll_steps=roll_steps, map_dev=map_dev)


REL2 = ((1.25, 0.8), (0.8, 1.2), (1.15, 1.3))
REL1 = ((1.3,), (0.7,), (1.15,))
CASES = [
    # S: one workgroup that is its own reducer; one or two workgroups round 256; four workgroups with a tail
    _case("s1", "pendulum", 1, 8, "none", (), 3, 2, 2101),
    _case("s255", "pendulum", 255, 8, "extended", ("length", "mass"), 3, 3, 2102, true_rel=REL2),
    _case("s256_d30", "pendulum", 256, 30, "single", ("length",), 3, 3, 2103, true_rel=REL1),  # D = 30: nq = 8
    _case("s257_edge", "pendulum", 257, 8, "extended", ("length", "mass"), 3, 3, 2104, true_rel=REL2, a_seq0="edge"),  # a start ON the bounds
    _case("s1021_ut", "pendulum", 1021, 8, "ut", ("length",), 2, 2, 2105, true_rel=REL1),
    # D = 1 (nq = 256) with roll_steps = 1: the whole sequence becomes zeros; D = 128 (nq = 2)
    _case("d1", "pendulum", 64, 1, "none", (), 3, 2, 2106),
    _case("d128", "pendulum", 64, 128, "none", (), 2, 2, 2107),
    # da = 2 with a full 2 x 2 a_cov, roll_steps = 3
    _case("skid_cov", "skid", 63, 8, "extended", ("x_icr",), 3, 2, 2108, true_rel=((1.4,), (0.6,)), roll_steps=3, a_cov=FULL_COV),
    _case("nav_lds", "skid", 64, 8, "single", ("x_icr",), 2, 2, 2109, true_rel=((1.4,), (0.6,)), nav=True),
    _case("nav_dev", "skid", 64, 8, "single", ("x_icr",), 2, 2, 2109, true_rel=((1.4,), (0.6,)), nav=True, map_dev=True),
    _case("cart_ut", "cartpole", 64, 8, "ut", ("mass_pole", "length"), 3, 2, 2110, true_rel=((1.4, 0.6), (0.6, 1.4))),
    # environment 1 starts inside the obstacle at (-2, -6): the plant's collision freeze
    _case("part", "particle", 65, 10, "extended", ("mass",), 3, 3, 2111, true_rel=((1.4,), (0.7,), (1.2,)),
          start=((-3.3, -7.3, 4.0, 3.0), (-2.0, -6.0, 1.0, -2.0), (4.4, 0.3, -3.0, 4.5))),
]
BY_ID = {c["id"]: c for c in CASES}
IDS = [c["id"] for c in CASES]
# the dual episode's plant check (tests/test_gpu_amppi_dual_episode.py): its scenario's shape; in BY_ID for measure(), not among the IDS
DUAL_PLANT = _case("dual_plant", "pendulum", 257, 12, "extended", ("length", "mass"), 3, 3, 2201, true_rel=REL2)
BY_ID[DUAL_PLANT["id"]] = DUAL_PLANT

nav_map = sec.nav_map
family = sec.family
start_states = sec.start_states
plant_rows = sec.plant_rows
plant_step = sec.plant_step
variant_steps = sec.variant_steps
restated_loop = sec.restated_loop


def context_kwargs(case, **kw):
    """Context keywords of the case's prototype (the map comes beside them: Context(grid=))"""
    return ac.context_kwargs(case, **dict(dict(seed=case["seed"], **(NAV if case["nav"] else {})), **kw))


def param_rows(case):
    """1 ("single"), S ("extended"), 2P + 1 (sigma points) or 0 ("none") parameter rows per environment and period"""
    return {"none": 0, "single": 1, "extended": case["S"], "ut": 2 * len(case["up"]) + 1}[case["mode"]]


def tick_params(case, T=None, B=None):
    """[T, B, rows, P] fp32 parameter rows round the nominal row, every (t, b, row) another draw; the sigma-point mode: the mean of
    environment b, moved by 3 % per environment, and the mean -+ one standard deviation per column; None in the "none" mode"""
    rows = param_rows(case)
    if not rows:
        return None
    T, B = case["T"] if T is None else T, case["B"] if B is None else B
    nom, P = sec.nominal_row(case), len(case["up"])
    if case["mode"] == "ut":
        mean = nom[None] * (1.0 + 0.03 * np.arange(B, dtype=np.float32))[:, None]  # [B, P]
        off = np.concatenate((np.zeros((1, P)), np.eye(P), -np.eye(P))) * (ac.REL_STD * nom)  # [2P + 1, P]
        return np.broadcast_to((mean[:, None] + off[None]).astype(np.float32), (T, B, rows, P)).copy()
    rng = np.random.default_rng(case["seed"] + 7)
    return (nom * (1.0 + ac.REL_STD * rng.standard_normal((T, B, rows, P)))).astype(np.float32)


def start_sequences(case, B=None):
    """[B, H, da] fp32 nominal sequences, every environment its own; "edge": ON the action bounds, alternating"""
    f = family(case)
    B = case["B"] if B is None else B
    H, da = case["H"], f["da"]
    if case.get("a_seq0") == "edge":
        one = (np.asarray(f["hi"], np.float32) * np.where(np.arange(H) % 2 == 0, 1.0, -1.0)[:, None]).astype(np.float32)
        return np.stack([one if b % 2 == 0 else -one for b in range(B)])
    rng = np.random.default_rng(case["seed"] + 3)
    return (f["a_scale"] * rng.standard_normal((B, H, da))).astype(np.float32)


def variants_of(case):
    """the wrong plants the case can show: no true row without uncertain parameters, no previous period at T = 1"""
    return {"unstepped"} | ({"nominal"} if case["up"] else set()) | ({"prev_action"} if case["T"] > 1 else set())


_measured = {}


def measure(cid, grid=None):
    """(d, tol, {variant: distance in tolerances}) of a case from the restatement alone (svmpc_episode_cases.measure on this table)"""
    if cid in _measured:
        return _measured[cid]
    case = BY_ID[cid]
    xs, acts, exact = restated_loop(case, grid)
    rows = plant_rows(case)
    T = acts.shape[0]
    f32 = np.stack([plant_step(case, xs[t], acts[t], rows, grid, dtype=np.float32) for t in range(T)])
    moved = np.stack([plant_step(case, sec.ulp_moved(xs[t], case["seed"] + t), acts[t], rows, grid) for t in range(T)])
    d = max(elemerr(f32, exact), elemerr(moved, exact))
    tol = max(TOL_FLOOR, 2.0 * d)
    power = distances(case, xs[1:], xs[:-1], acts, rows, grid, tol)
    _measured[cid] = (d, tol, power)
    return _measured[cid]


def distances(case, stepped, prev, acts, rows, grid, tol):
    """{variant: the LARGEST distance over the periods, in tolerances, between the states `stepped` [T, B, ds] and the wrong plant on
    (prev[t], acts[t])}: a wrong plant shows in at least one period"""
    out = {}
    for t in range(acts.shape[0]):
        for k, v in variant_steps(case, prev[t], acts[t], acts[t - 1] if t else None, rows, grid).items():
            out[k] = max(out.get(k, 0.0), elemerr(stepped[t], v) / tol)
    return out


def plant_tolerance(case, grid=None):
    d, tol, _ = measure(case["id"], grid)
    assert tol <= TOL_CAP, (case["id"], d)
    return tol
