"""Cases and the float64 restatement (TEST INFRASTRUCTURE) of the batched MultiDISCO (csrc/disco_batch.hpp, dust_disco_batch_*), shared by
tests/test_disco_batch_cpu.py, tests/test_gpu_disco_batch.py and tests/test_gpu_disco_episode.py.  Data and seeded numpy only: nothing here
imports the library.

A case is an AMPPI scenario dict (tests/amppi_cases.py `A`), so that the plant constants of the device context (`amppi_cases.context_kwargs`)
and of the float64 model step and costs (`amppi_cases._step` / `_costs`, imported - never copied) are the same numbers, plus the sizes
N, M, the step's strategy and `steps`, ctrl_penalty and the environments B.

The restatement follows the reference line by line (dust/controllers/disco.py:139-417):
  rollout_costs   the N S M rollouts and their state costs - the mean over the M rows, or (sigma) the weighted sum in which entry (m, t) of
                  a rollout's flat [point][step] block meets weight (m H + t) mod pts (disco.py:312-323);
  forward         the control cost a_reg sum -(a - a_seq) (a_mat a_pre), beta = the GLOBAL minimum, omega, eta, a_mat += sum omega eps,
                  a_mix = softmax(eta) - from given state costs and actions, in any dtype;
  step            a_seq by strategy (the FIRST maximum; "argmax" clamps that row of a_mat in place: a view, disco.py:401, 410), the clamp,
                  next_actions, the roll of a_seq and a_mat by `steps` with zeros behind.
`dtype=np.float32` evaluates the same statements on fp32 operands with the sums over S taken sequentially: the distance between the two
evaluations of a case is what `stage_tolerance` is made of (the project's rule, DESIGN.md section 2: tol = max(floor, 2 d)), never device
output.  The `variant=` arguments restate the wrong forms a test must keep away from.
"""
import numpy as np

import amppi_cases as ac
from helpers import elemerr

TOL_FLOOR = 1e-5
STRATEGIES = ("argmax", "average", "external")


def _case(tag, family, N, S, M, H, up, seed, strategy="average", steps=1, ctrl_penalty=1.0, sigma=False, nav=False, B=3, tie=False, T=3, start=None):
    mode = "ut" if sigma else ("extended" if up else "none")
    return dict(ac.A("disco_" + tag, family, S, H, mode, up, seed), id=tag, N=N, M=2 * len(up) + 1 if sigma else M, strategy=strategy, steps=steps,
                ctrl_penalty=ctrl_penalty, sigma=sigma, nav=nav, B=B, tie=tie, T=T, start=start)


CASES = [
    _case("one", "pendulum", 1, 1, 1, 1, (), 2101, B=1, T=1),                                        # every bound at 1
    _case("mppi", "pendulum", 1, 128, 1, 8, (), 2102),                                               # the MPPI baseline
    _case("disco", "pendulum", 1, 64, 5, 8, ("length", "mass"), 2103, sigma=True),                  # the DISCO case: 5 points, P 2
    _case("multi_avg", "pendulum", 4, 16, 2, 8, ("length",), 2104, steps=2, ctrl_penalty=0.4),      # the shape of disco_mppi
    _case("multi_arg", "pendulum", 4, 16, 2, 8, ("length",), 2105, strategy="argmax", steps=2, ctrl_penalty=0.4),
    _case("wave63", "pendulum", 3, 63, 8, 6, ("length", "mass"), 2106, strategy="argmax"),           # a partial wave, G > 1 groups
    _case("wave257", "pendulum", 3, 257, 8, 6, ("length", "mass"), 2107),
    # two action channels on the demo's map.  The starts are those of tests/svmpc_sim_cases.py `part` (environment 0 just left of the block
    # at x = -3.1 .. -0.9 and heading into it: it crashes in period 0 whatever the action; environment 1 inside the goal radius;
    # environment 3 within reach of neither), and environment 2 one cell further left: the first step moves a position by the OLD velocity,
    # so it is free after period 0 and on the block after period 1 (tests/test_disco_batch_cpu.py proves both from the float64 step)
    _case("part", "particle", 2, 32, 1, 6, (), 2108, strategy="argmax", B=4,
          start=((-3.15, -6.03, 4.0, 0.5), (8.8, 8.9, 0.1, -0.1), (-3.21, -6.03, 4.0, 0.5), (4.4, 0.3, -3.0, 4.5))),
    _case("skid", "skid", 2, 32, 2, 6, ("x_icr",), 2109),
    _case("skid_nav_sigma", "skid", 2, 32, 7, 6, ("x_icr", "wheel_radius", "axial_distance"), 2110, sigma=True, nav=True, B=2),  # P 3: 7 points
    _case("skid_sigma", "skid", 2, 32, 7, 6, ("x_icr", "wheel_radius", "axial_distance"), 2115, sigma=True, B=2),  # ... without the map
    _case("cart", "cartpole", 2, 32, 2, 6, ("mass_pole", "length"), 2111, strategy="argmax", B=2),
    _case("all_out", "pendulum", 2, 16, 1, 5, (), 2112, steps=5, B=2, T=1),                          # steps = H: everything rolls out
    _case("tie", "pendulum", 2, 16, 1, 5, (), 2113, strategy="argmax", tie=True, B=2, T=1),          # an exact tie of a_mix: index 0
    _case("corner", "pendulum", 64, 8, 1, 128, (), 2114, strategy="argmax", steps=3, B=2, T=1),      # N 64 x D 128: the box's corner
]
BY_ID = {c["id"]: c for c in CASES}
IDS = [c["id"] for c in CASES]
# The episodes (tests/test_gpu_disco_episode.py): the cases run as T closed-loop periods, and the reference's rules each runs under - goal
# [ds] and radius, stop_on_crash.  EVENTS: what `part` forces, {environment: (period, status)}; the other cases' goals are out of reach (a
# rule that is on and never fires), and wherever a rule does fire the device must agree with the fp32 replicas of tests/svmpc_sim_cases.py.
EPISODE_IDS = ["one", "mppi", "disco", "multi_arg", "part", "skid", "skid_nav_sigma", "cart"]
RULES = {
    "one": dict(goal=None, radius=None, crash=False),
    "mppi": dict(goal=(0.0, 0.0), radius=0.5, crash=False),
    "disco": dict(goal=(0.0, 0.0), radius=0.5, crash=False),
    "multi_arg": dict(goal=None, radius=None, crash=False),
    "part": dict(goal=ac.PART["target"], radius=1.0, crash=True),
    "skid": dict(goal=ac.SKID["goal"], radius=0.05, crash=False),
    "skid_nav_sigma": dict(goal=ac.SKID["goal"], radius=0.05, crash=True),
    "cart": dict(goal=ac.CART["goal"], radius=0.1, crash=False),
}
EVENTS = {"part": {0: (0, 2), 1: (0, 1), 2: (1, 2)}}
NAV = dict(w_obs=10.0, cell_size=0.02)


def nav_map():
    """[80, 80] 0 / 1 occupancy in blocks of 2 cells of 0.02 m (200 words: staged into LDS)"""
    rng = np.random.default_rng(7)
    return np.ascontiguousarray(np.kron((rng.random((40, 40)) < 0.4).astype(np.float32), np.ones((2, 2), np.float32)))


def family(case):
    return ac.FAMILY[case["family"]]


def context_kwargs(case, **kw):
    """Context keywords of the case's prototype (a map comes beside them: Context(grid=); sigma weights: set_param_weights)"""
    return ac.context_kwargs(case, **dict(dict(N=case["N"], M=case["M"], seed=case["seed"], ctrl_penalty=case["ctrl_penalty"],
                                               **(NAV if case["nav"] else {})), **kw))


def sigma_weights(case):
    """(loc_weights [pts] float64, lambda + n) of the case's transform"""
    return ac.weights(len(case["up"]))


def sigma_points(case, shift=0.0):
    """[pts, P] fp32: the mean, then mean +- sqrt(lambda + n) std e_i of the case's diagonal parameter distribution (utf.py:93-118)"""
    mean, std = ac.dist_of(case)
    mean = (mean * np.float32(1.0 + shift)).astype(np.float32)
    P = len(case["up"])
    root = np.float32(np.sqrt(sigma_weights(case)[1]))
    pts = [mean] + [mean + root * std * np.eye(P, dtype=np.float32)[i] for i in range(P)] + [mean - root * std * np.eye(P, dtype=np.float32)[i] for i in range(P)]
    return np.stack(pts).astype(np.float32)


def inputs(case, B=None):
    """every environment's own state, a_mat, a_seq, recorded actions (drawn around a_mat), parameter rows, external rows and seed"""
    f = family(case)
    B = case["B"] if B is None else B
    N, S, M, H, da = case["N"], case["S"], case["M"], case["H"], f["da"]
    rng = np.random.default_rng(case["seed"])
    st0 = np.asarray(f["state0"], np.float32)
    states = np.stack([(st0 + np.float32(0.05 * b) * np.arange(1, f["ds"] + 1, dtype=np.float32)).astype(np.float32) for b in range(B)])
    if case["start"] is not None:
        states = np.asarray(case["start"], np.float32)[:B]
    a_mat = (f["a_scale"] * rng.standard_normal((B, N, H, da))).astype(np.float32)
    a_seq = (f["a_scale"] * rng.standard_normal((B, H, da))).astype(np.float32)
    chol = np.sqrt(np.diag(ac.a_cov_of(case))).astype(np.float32)
    z = rng.standard_normal((B, S, N, H, da)).astype(np.float32)
    if case["tie"]:  # two policies with identical rows and identical recorded actions
        a_mat[:, 1] = a_mat[:, 0]
        z[:, :, 1] = z[:, :, 0]
    actions = (a_mat[:, None] + chol * z).astype(np.float32)
    ext = (2.0 * np.asarray(f["hi"], np.float32) * rng.standard_normal((B, H, da))).astype(np.float32)  # (some entries beyond the bounds)
    params = None
    if case["sigma"]:
        params = np.stack([sigma_points(case, 0.03 * b) for b in range(B)])
    elif case["up"]:
        mean, std = ac.dist_of(case)
        params = (mean + std * rng.standard_normal((B, M, len(case["up"])))).astype(np.float32)
    return dict(states=states, a_mat=a_mat, a_seq=a_seq, actions=actions, ext=ext, params=params, seeds=[case["seed"] + 13 * b for b in range(B)])


def plant_rows(case, B=None):
    """[B, P] fp32 true parameter rows (None without uncertain parameters)"""
    if not case["up"]:
        return None
    B = case["B"] if B is None else B
    mean, _ = ac.dist_of(case)
    rel = np.array([[1.0 + 0.2 * ((b + j) % 3 - 1) for j in range(len(case["up"]))] for b in range(B)], np.float32)
    return (mean[None] * rel).astype(np.float32)


def episode_params(case, T, B=None):
    """[T, B, M, P] fp32 parameter rows of T periods (the sigma points of a prior that moves a little per period); None without parameters"""
    if not case["up"]:
        return None
    B = case["B"] if B is None else B
    if case["sigma"]:
        return np.stack([np.stack([sigma_points(case, 0.03 * b + 0.01 * t) for b in range(B)]) for t in range(T)])
    mean, std = ac.dist_of(case)
    rng = np.random.default_rng(case["seed"] + 7)
    return (mean + std * rng.standard_normal((T, B, case["M"], len(case["up"])))).astype(np.float32)


# ------------------------------------------------------------------------------------------------ float64 restatement
def rollout_costs(case, state, actions, params, grid=None, uniform_weights=False, dtype=np.float64):
    """state costs [S, N] of one environment in `dtype`: state [ds], actions [S, N, H, da], params [M, P] or None.  Families whose
    instantaneous cost has no action term (Pendulum; skid-steer and cart-pole with a zero control weight), and Particle, whose cost adds
    sum w_ctrl a^2 of the raw action (particle.py:170-198)."""
    f = family(case)
    S, N, M, H, ds = case["S"], case["N"], case["M"], case["H"], f["ds"]
    acts = np.asarray(actions, dtype).reshape(S * N, H, f["da"])
    total = np.zeros((M, S * N), dtype)
    inst_mt = np.zeros((M, S * N, H), dtype)
    term_m = np.zeros((M, S * N), dtype)
    for m in range(M):
        p = dict(f["defaults"])
        if params is not None:
            for j, k in enumerate(case["up"]):
                p[k] = np.full((S * N, 1), np.asarray(params, np.float32)[m, j], np.float32 if case["sigma"] else dtype)
        # forward() casts the state to fp32 and expands it into an fp32 tensor (disco.py:369, 190): the FIRST step reads fp32 operands -
        # what it computes of the state alone (the trigonometry) is fp32 arithmetic whatever the default dtype; its result, and the
        # tensor the costs read, are promoted
        x = np.repeat(np.asarray(state, np.float32)[None], S * N, 0)
        for t in range(H):
            inst_mt[m, :, t] = ac._costs(case, x.astype(dtype), grid, False)  # the state BEFORE the action (disco.py:306)
            if case["family"] == "particle":
                inst_mt[m, :, t] += (acts[:, t] * acts[:, t] * np.asarray(f["w_ctrl"], dtype)).sum(-1)
            x = (_first_pendulum_step(case, x, acts[:, t], p) if (t == 0 and case["family"] == "pendulum" and dtype == np.float64)
                 else ac._step(case, x, acts[:, t], p, grid)).astype(dtype)
        term_m[m] = ac._costs(case, x, grid, True)
        total[m] = inst_mt[m].sum(-1) + term_m[m]
    if not case["sigma"]:
        return (_seq_sum(total, dtype) / dtype(M)).astype(dtype).reshape(S, N)
    w = (np.full(M, 1.0 / M) if uniform_weights else sigma_weights(case)[0]).astype(dtype)
    idx = (np.arange(M)[:, None] * H + np.arange(H)[None]) % M  # entry (m, t) meets weight (m H + t) mod pts
    return ((inst_mt * w[idx][:, None, :]).sum((0, 2), dtype=dtype) + (term_m * w[:, None]).sum(0, dtype=dtype)).astype(dtype).reshape(S, N)


def _first_pendulum_step(case, x32, a, p):
    """amppi_cases._step's Pendulum statement for the fp32 first step of a float64 run, with the fp32 sine taken by torch - the
    reference's own: numpy's fp32 sine differs from it by an ulp in some arguments, 1e-10 of a cost"""
    import math

    import torch

    f = family(case)
    dt = f["dt"]
    th, thd = x32[:, :1], x32[:, 1:]
    g, m, ln = p["g"], p["mass"], p["length"]
    u = np.clip(a, f["lo"][0], f["hi"][0])
    sn = torch.sin(torch.from_numpy(np.ascontiguousarray(th)) + math.pi).numpy()
    thd = thd + dt * ((1.0 / (2 * ln)) * (-3 * g) * sn + (1.0 / (m * ln ** 2)) * 3.0 * u)
    thd = np.clip(thd, -f["max_speed"], f["max_speed"])
    return np.concatenate((th + thd * dt, thd), 1)


def _seq_sum(x, dtype):
    """sum over axis 0 in `dtype`, sequentially (the order of a lane's loop), for fp32; float64: numpy's"""
    if dtype == np.float64:
        return x.sum(0)
    acc = np.zeros(x.shape[1:], dtype)
    for row in x:
        acc = (acc + row).astype(dtype)
    return acc


def forward(case, a_mat, a_seq, actions, state_costs, around_a_mat, dtype=np.float64, variant=None):
    """MultiDISCO.forward from the rollouts' state costs [S, N] on: -> dict(costs [S, N], omega [S, N], eta [N] on the reference's scale,
    a_mix [N], a_mat [N, H, da]).  around_a_mat: eps = actions - a_mat (drawn actions), else actions - a_seq (recorded ones).
    variant: "noctrl" (control cost dropped), "wrong_base" (eps around the other base), "unshifted" (a_mix from eta under per-policy
    minima, never carried back to the global beta)."""
    f = family(case)
    t = dtype
    temp = t(f["lam"])
    a_reg = t(f["lam"] * (1.0 - case["ctrl_penalty"]))  # temperature * (1 - ctrl_penalty) in Python floats (disco.py:90), then the dtype
    a_mat, a_seq, acts = np.asarray(a_mat, t), np.asarray(a_seq, t), np.asarray(actions, t)
    pre = (t(1.0) / np.diag(ac.a_cov_of(case)).astype(t)).astype(t)  # torch.inverse(a_cov) of a diagonal a_cov, in the dtype
    costs = np.asarray(state_costs, t)
    if a_reg != 0 and variant != "noctrl":  # disco.py:338-344: eps = actions - a_seq here, whatever drew the actions
        e = acts - a_seq[None, None]
        costs = (costs + a_reg * ((-e) * (a_mat * pre)[None]).sum((-2, -1), dtype=t)).astype(t)
    if variant == "wrong_base":
        around_a_mat = not around_a_mat
    eps = acts - (a_mat[None] if around_a_mat else a_seq[None, None])
    beta = costs.min(0, keepdims=True) if variant == "unshifted" else costs.min()
    lc = (t(-1) * (costs - beta) / temp).astype(t)
    mx = lc.max(0)
    eta = (mx + np.log(_seq_sum(np.exp(lc - mx).astype(t), t))).astype(t)
    omega = np.exp(lc - eta).astype(t)
    delta = _seq_sum((omega[:, :, None, None] * eps).astype(t), t)
    lse = eta.max() + np.log(np.exp(eta - eta.max()).sum(dtype=t))
    return dict(costs=costs, omega=omega, eta=eta, a_mix=np.exp(eta - lse).astype(t), a_mat=(a_mat + delta).astype(t))


def step(case, a_mat, a_seq, a_mix, strategy, steps, ext=None, dtype=np.float64, variant=None):
    """MultiDISCO.step -> dict(next [steps, da], a_seq [H, da], a_mat [N, H, da]).  variant: "swapped" (the other strategy), "roll_one"
    (rolled by one instead of `steps`), "last_max" (the LAST maximum of a_mix)."""
    f = family(case)
    t = dtype
    a_mat, a_mix = np.array(a_mat, t), np.asarray(a_mix, t)
    lo, hi = np.asarray(f["lo"], t), np.asarray(f["hi"], t)
    if variant == "swapped":
        strategy = "average" if strategy == "argmax" else "argmax"
    if strategy == "argmax":
        i = int(np.argmax(a_mix)) if variant != "last_max" else int(len(a_mix) - 1 - np.argmax(a_mix[::-1]))
        a_mat[i] = np.clip(a_mat[i], lo, hi)  # (a view in the reference: the clamp reaches a_mat)
        seq = a_mat[i].copy()
    elif strategy == "average":
        seq = np.clip(np.tensordot(a_mix, a_mat, 1).astype(t), lo, hi)
    else:
        seq = np.clip(np.asarray(ext, t), lo, hi)
    sh = 1 if variant == "roll_one" else steps
    new_seq, new_mat = np.zeros_like(seq), np.zeros_like(a_mat)
    new_seq[:seq.shape[0] - sh] = seq[sh:]
    new_mat[:, :seq.shape[0] - sh] = a_mat[:, sh:]
    return dict(next=seq[:steps].copy(), a_seq=new_seq, a_mat=new_mat)


STAGES = ("omega", "a_mat1", "a_mix", "next", "a_seq", "a_mat")  # forward's, then step's (a_mat1: before the roll)


def stages(case, a_mat, a_seq, actions, costs_with_ctrl, around_a_mat, ext=None, dtype=np.float64):
    """every stage downstream of given FINAL costs (control cost included: the device's own COSTS record) in `dtype`"""
    nc = dict(case, ctrl_penalty=1.0)
    fw = forward(nc, a_mat, a_seq, actions, costs_with_ctrl, around_a_mat, dtype)
    st = step(case, fw["a_mat"], a_seq, fw["a_mix"], case["strategy"], case["steps"], ext, dtype)
    return dict(omega=fw["omega"], a_mat1=fw["a_mat"], a_mix=fw["a_mix"], next=st["next"], a_seq=st["a_seq"], a_mat=st["a_mat"])


def synthetic_costs(case, b=0):
    """[S, N] fp32 costs of the scale the case's rollouts have - for tolerances measured without a device or a model"""
    rng = np.random.default_rng(case["seed"] + 101 + b)
    lam = family(case)["lam"]
    return (lam * (2.0 + np.abs(rng.standard_normal((case["S"], case["N"]))))).astype(np.float32)


_measured = {}


def stage_tolerance(case):
    """{stage: tol} from the restatement alone: d = the distance between the fp32 and the float64 evaluation of the case's stages on its own
    inputs and on costs of its scale (and on costs moved one fp32 ulp: the device's costs are rounded ones), tol = max(TOL_FLOOR, 2 d)"""
    if case["id"] in _measured:
        return _measured[case["id"]]
    inp = inputs(case)
    d = {k: 0.0 for k in STAGES}
    for b in range(case["B"]):
        c = synthetic_costs(case, b)
        if case["tie"]:
            c[:, 1] = c[:, 0]
        up = np.random.default_rng(case["seed"] + 5).random(c.shape) < 0.5
        if case["tie"]:
            up[:, 1] = up[:, 0]
        moved = np.where(up, np.nextafter(c, np.float32(np.inf)), np.nextafter(c, np.float32(-np.inf))).astype(np.float32)
        args = (inp["a_mat"][b], inp["a_seq"][b], inp["actions"][b])
        exact = stages(case, *args, c, True, inp["ext"][b])
        for other in (stages(case, *args, c, True, inp["ext"][b], np.float32), stages(case, *args, moved, True, inp["ext"][b])):
            for k in STAGES:
                d[k] = max(d[k], elemerr(other[k], exact[k]))
    _measured[case["id"]] = {k: max(TOL_FLOOR, 2.0 * v) for k, v in d.items()}
    return _measured[case["id"]]


def final_costs(case, inp, b, grid=None, dtype=np.float64, variant=None, uniform_weights=False):
    """environment b's costs [S, N] as forward() softmaxes them - rollouts, then the control cost - on the recorded actions"""
    sc = rollout_costs(case, inp["states"][b], inp["actions"][b], None if inp["params"] is None else inp["params"][b], grid, uniform_weights, dtype)
    return forward(case, inp["a_mat"][b], inp["a_seq"][b], inp["actions"][b], sc, False, dtype, variant)["costs"]


_cost_measured = {}


def cost_tolerance(case, grid=None):
    """the tolerance of the COSTS record against the float64 rollouts, from the restatement alone: d = the distance between the fp32 and
    the float64 evaluation of every environment's costs, tol = max(TOL_FLOOR, 2 d)"""
    if case["id"] not in _cost_measured:
        inp = inputs(case)
        d = max(elemerr(final_costs(case, inp, b, grid, np.float32), final_costs(case, inp, b, grid)) for b in range(case["B"]))
        _cost_measured[case["id"]] = max(TOL_FLOOR, 2.0 * d)
    return _cost_measured[case["id"]]


# ------------------------------------------------------------------------------------------------ the closed loop of the fixtures
# tests/golden/make_golden_disco_loop.py runs these cases through the reference's own MultiDISCO: LOOP_T periods of forward (its draws
# recorded: eps = chol_a z), step(strategy, steps) and the reference plant under the environment's true row.
LOOP_IDS = ["mppi", "disco", "multi_avg", "multi_arg", "part", "skid", "skid_sigma", "cart"]
LOOP_T = 4
LOOP_ENV = 1  # the case's environment the fixture runs (state, a_mat, a_seq, true row)
LOOP_QUANT = ("costs", "omega", "a_mat1", "a_mix", "next", "a_seq", "a_mat", "plant")


def loop_err(g, q, k, got, ref=None):
    """the distance of `got` from period k of the fixture's quantity q (or from `ref`): element-wise, and for `next` - steps x da numbers,
    often one, sometimes next to zero - with the RMS of the period's plan a_mat1 as the absolute floor (stored as floor_next [T])"""
    ref = g[q][k] if ref is None else ref
    return elemerr(got, ref, floor=float(g["floor_next"][k])) if q == "next" else elemerr(got, ref)


# the wrong forms a fixture stores beside the right quantity: name -> (the quantity it replaces, whether the case can show it)
OFF = {
    "swapped": ("next", lambda c: c["N"] > 1),                  # strategies swapped
    "noctrl": ("costs", lambda c: c["ctrl_penalty"] != 1.0),    # control cost dropped
    "roll_one": ("a_mat", lambda c: 1 < c["steps"] < c["H"]),   # rolled by one instead of `steps`
    "wrong_base": ("a_mat1", lambda c: True),                   # eps around the wrong base
    "unshifted": ("a_mix", lambda c: c["N"] > 1),               # a_mix from eta under per-policy minima
    "uniform": ("costs", lambda c: c["sigma"]),                 # sigma weights uniform
}


def loop_inputs(case):
    """the fixture's inputs: state [ds], a_mat0 [N, H, da], a_seq0 [H, da], z [T, S, N, H, da] standard normal draws, params [T, M, P]
    (sampled rows per period), or dist_mean / dist_std [P] (sigma points), true [P] (the plant's row), all fp32"""
    inp, e = inputs(case), LOOP_ENV
    f = family(case)
    rng = np.random.default_rng(case["seed"] + 500)
    out = dict(state=inp["states"][e], a_mat0=inp["a_mat"][e], a_seq0=inp["a_seq"][e],
               z=rng.standard_normal((LOOP_T, case["S"], case["N"], case["H"], f["da"])).astype(np.float32))
    if case["sigma"]:
        out["dist_mean"], out["dist_std"] = ac.dist_of(case)
    elif case["up"]:
        mean, std = ac.dist_of(case)
        out["params"] = (mean + std * rng.standard_normal((LOOP_T, case["M"], len(case["up"])))).astype(np.float32)
    if case["up"]:
        out["true"] = plant_rows(case)[e]
    return out


def loop_grid(case):
    if case["family"] != "particle":
        return None
    from oracle import grid_4x4_map

    return grid_4x4_map()


def restate_period(case, state, a_mat, a_seq, z, rows, true, grid, variant=None):
    """one period in float64 from float64 / fp32 operands -> dict of LOOP_QUANT (+ actions); variant: a key of OFF"""
    f = family(case)
    chol = np.sqrt(np.diag(ac.a_cov_of(case)).astype(np.float64))
    acts = a_mat[None] + chol * np.asarray(z, np.float64)
    sc = rollout_costs(case, state, acts, rows, grid, uniform_weights=variant == "uniform")
    fw = forward(case, a_mat, a_seq, acts, sc, True, variant=variant if variant in ("noctrl", "wrong_base", "unshifted") else None)
    st = step(case, fw["a_mat"], a_seq, fw["a_mix"], case["strategy"], case["steps"], variant=variant if variant in ("swapped", "roll_one") else None)
    p = dict(f["defaults"])
    if true is not None:
        for j, k in enumerate(case["up"]):
            p[k] = np.full((1, 1), np.asarray(true, np.float32)[j], np.float64)
    plant = ac._step(case, np.asarray(state, np.float64)[None], st["next"][:1], p, grid)[0]
    return dict(costs=fw["costs"], omega=fw["omega"], a_mat1=fw["a_mat"], a_mix=fw["a_mix"], next=st["next"], a_seq=st["a_seq"], a_mat=st["a_mat"],
                plant=plant, actions=acts)


def loop_rows(case, inp, t, sigma_pts=None):
    return sigma_pts if case["sigma"] else (inp["params"][t] if "params" in inp else None)


def restate_loop(case, inp, sigma_pts=None):
    """the LOOP_T periods in float64, chained on themselves -> {quantity: [T, ...]}"""
    grid = loop_grid(case)
    state, a_mat, a_seq = (np.asarray(inp[k], np.float64) for k in ("state", "a_mat0", "a_seq0"))
    out = {k: [] for k in LOOP_QUANT}
    for t in range(LOOP_T):
        r = restate_period(case, state, a_mat, a_seq, inp["z"][t], loop_rows(case, inp, t, sigma_pts), inp.get("true"), grid)
        for k in LOOP_QUANT:
            out[k].append(r[k])
        state, a_mat, a_seq = r["plant"], r["a_mat"], r["a_seq"]
    return {k: np.stack(v) for k, v in out.items()}


def restate_off(case, inp, twin, sigma_pts=None):
    """every wrong form the case can show, per period from the float64 twin's OWN previous period (first-divergence form)
    -> {"<quantity>_off_<name>": [T, ...]}"""
    grid = loop_grid(case)
    out = {}
    for name, (q, shows) in OFF.items():
        if not shows(case):
            continue
        rows = []
        for t in range(LOOP_T):
            state = inp["state"] if t == 0 else twin["plant"][t - 1]
            a_mat = inp["a_mat0"] if t == 0 else twin["a_mat"][t - 1]
            a_seq = inp["a_seq0"] if t == 0 else twin["a_seq"][t - 1]
            rows.append(restate_period(case, np.asarray(state, np.float64), np.asarray(a_mat, np.float64), np.asarray(a_seq, np.float64), inp["z"][t],
                                       loop_rows(case, inp, t, sigma_pts), inp.get("true"), grid, variant=name)[q])
        out["%s_off_%s" % (q, name)] = np.stack(rows)
    return out
