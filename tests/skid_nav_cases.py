"""Skid-steer navigation scenarios (TEST INFRASTRUCTURE): the reference's MultiDISCO.forward and AMPPI.update_actions on its SkidSteerRobot
with the navigation cost - the quadratic family plus w_obs * obst_map.get_collisions(states[..., 0:2]), the obstacle term of
Particle.default_inst_cost / default_term_cost (particle.py:170-225).  Shared by tests/golden/make_golden_skid_nav.py, which runs the
reference on them, and by the tests that read tests/golden/skid_nav_<tag>.npz and amppi_nav_<tag>.npz.  Data and seeded numpy only: nothing
here imports the reference or the library.

Scenario dicts.  Both kinds: tag, H, up (uncertain parameter names in column order), fixed (x_icr, wheel_radius, axial_distance), bounds
(wheel speeds), dt, a_cov (None: SIGMA_A^2 I), cell, map_dim (metres, even; the map has map_dim / cell cells a side), p_occ (share of
occupied blocks), w_obs, fwd (mean wheel-speed command), state0, seed (the base of the generator's seed search), offs (the `_off`
variants of the costs the fixture carries).
  kind "disco" (ROLLOUTS): N, S, M, dist / lo / hi / loc / scale / log as tests/skid_cases.py, ctrl_penalty, a_seq, w_ctrl;
  kind "ut" (ROLLOUTS): N, S, the 2P + 1 sigma points of a normal around the defaults with REL_STD, alpha (MerweScaledUTF);
  kind "amppi" (AMPPI): S, mode ("none" / "single" / "extended" / "ut"), a_seq0 ("edge": on the action bounds).
The occupancy map is drawn here (make_map): blocks of BLOCK x BLOCK cells, each occupied with probability p_occ, from the scenario's own
map seed - so a fixture stores it bit-packed (pack_map / unpack_map) and the generator asserts that it is this one.

Conditions a fixture must meet are the generator's (its docstring); the float64 restatements below (restate_disco, restate_amppi)
reproduce the reference's float64 runs and give the `_off` variants their meaning (nav_terms).
"""
import math

import numpy as np

NAMES3 = ("x_icr", "wheel_radius", "axial_distance")  # params_dict order of SkidSteerRobot (skid_steer_robot.py:39-43)
DEFAULTS = dict(x_icr=0.2, wheel_radius=0.0625, axial_distance=0.475)  # SkidSteerRobot.__init__
BOUNDS = (-3.0, 3.0)
DT = 0.1
GOAL = (1.2, 0.6, 0.3, 0.0, 0.0)
W_STATE = (2.0, 2.0, 0.5, 0.1, 0.05)
W_TERM = (20.0, 20.0, 2.0, 0.0, 0.0)
W_CTRL = (0.03, 0.02)
STATE0 = (0.33, -0.24, 0.4, 0.1, -0.05)  # mid-cell at cells of 0.1 and of 0.05 (tests/skid_cases.py STATE0 = (0.3, ...) lies ON an edge)
SIGMA_A = 1.0
TEMPERATURE = 20.0  # costs of 20 .. 200: (max - min) / temperature stays below 10, the fp32 softmax keeps its digits
FULL_COV = ((1.0, 0.3), (0.3, 0.64))
CTRL_PENALTY = 0.6
REL_STD = 0.1
UT_ALPHA = 1.0  # MerweScaledUTF(alpha=): weights (0, 1 / 2n, ...) - alpha = 0.5 gives (-3, 2, 2) at n = 1, seven times the rounding
BLOCK = 3
TOL, CAP = 1e-5, 5e-5
MARGIN = 1e-4     # cells: every state's scaled position keeps this distance from an integer, on both axes
MARGIN_RATIO = 10.0  # ... and MARGIN_RATIO times the largest fp32 - float64 difference of that scaled position
MAX_TRIES = 500
TWIN_SCALE = 65536.0
VARIANTS = ("w0", "transpose", "round", "noterm", "shift", "free")


def _S(kind, tag, seed, **kw):
    d = dict(kind=kind, tag=tag, seed=seed, H=10, up=(), dist=None, log=False, fixed=dict(DEFAULTS), bounds=BOUNDS, dt=DT, a_cov=None, cell=0.1,
             map_dim=(4, 4), p_occ=0.4, w_obs=10.0, fwd=1.5, state0=STATE0, offs=("w0", "transpose", "round", "noterm", "shift"), ctrl_penalty=1.0,
             a_seq=False, w_ctrl=(0.0, 0.0) if kind != "disco" else W_CTRL, M=1, N=1, mode="none", alpha=UT_ALPHA)
    d.update(kw)
    d["up"] = tuple(d["up"])
    d["fixed"] = dict(DEFAULTS, **d["fixed"])
    if kind == "ut":
        d["M"] = 2 * len(d["up"]) + 1
    return d


XW = dict(dist="uniform", lo=(0.1, 0.05), hi=(0.3, 0.08))
ROLLOUTS = [
    _S("disco", "nominal", 1100, N=6, S=16),  # 96 lanes
    # 37 x 9 = 333 lanes: one full 256-lane block and a partial one; D = 30: the last Philox block of a row is partial
    _S("disco", "ragged", 1200, N=37, S=9, H=15, M=2, up=("wheel_radius", "x_icr"), dist="uniform", lo=(0.05, 0.1), hi=(0.08, 0.3), cell=0.05, w_obs=5.0),
    _S("disco", "p3_log", 1300, N=6, S=16, M=4, up=("axial_distance", "x_icr", "wheel_radius"), dist="lognormal", log=True, loc=(-0.75, -1.6, -2.8),
       scale=(0.1, 0.2, 0.1)),
    # a scalar-event params_dist: rollout r uses params[r % M] (disco.py:177-179); N S = 77 is no multiple of M = 3
    _S("disco", "scalar", 1410, N=7, S=11, M=3, up=("axial_distance",), dist="scalar", loc=(0.475,), scale=(0.08,)),
    _S("disco", "areg", 1500, N=6, S=16, M=3, up=("x_icr", "wheel_radius"), ctrl_penalty=CTRL_PENALTY, a_seq=True, w_obs=20.0, **XW),
    _S("disco", "fullcov", 1600, N=6, S=16, M=3, up=("x_icr", "wheel_radius"), a_cov=FULL_COV, **XW),
    # trajectories leave a 2 m x 2 m map on both sides of both axes: policies drive forwards and backwards along a diagonal heading
    _S("disco", "offmap", 1700, N=8, S=12, H=15, cell=0.05, map_dim=(2, 2), fixed=dict(wheel_radius=0.1), fwd=2.2, alternate=True,
       state0=(0.03, -0.02, 0.8, 0.1, -0.05), offs=("w0", "transpose", "round", "noterm", "shift", "free")),
    # 400 x 400 cells = 5000 words: over the 4096 the kernels stage into LDS - the lookups read device memory
    _S("disco", "bigmap", 1800, N=6, S=16, cell=0.05, map_dim=(20, 20)),
    # the sigma-point form: P = 1 (3 points) and P = 3 (7 points); H = 10 is a multiple of neither
    _S("ut", "ut_p1", 1900, N=5, S=20, up=("axial_distance",)),
    _S("ut", "ut_p3", 2000, N=5, S=20, up=("x_icr", "wheel_radius", "axial_distance")),
]
AMPPI = [
    _S("amppi", "one", 3130, S=1, H=6, p_occ=0.8),
    _S("amppi", "wave", 3200, S=64),
    _S("amppi", "odd_257", 3300, S=257, H=11, cell=0.05),  # two workgroups, an odd horizon
    _S("amppi", "single", 3430, S=96, mode="single", up=("x_icr", "wheel_radius")),
    _S("amppi", "extended", 3500, S=96, mode="extended", up=("wheel_radius", "axial_distance"), a_cov=FULL_COV),
    _S("amppi", "ut_p2", 3600, S=64, mode="ut", up=("x_icr", "axial_distance")),
    _S("amppi", "edge", 3700, S=64, a_seq0="edge"),  # the start sequence on the action bounds
]
ROLLOUT_NAMES = [s["tag"] for s in ROLLOUTS]
AMPPI_NAMES = [s["tag"] for s in AMPPI]
ROLLOUT_BY_TAG = {s["tag"]: s for s in ROLLOUTS}
AMPPI_BY_TAG = {s["tag"]: s for s in AMPPI}
ROLLOUT_QUANT = ("costs", "states", "omega", "a_mat1", "a_mix")
AMPPI_QUANT = ("costs", "states", "omega", "a_seq1")
MIRROR_CASES = ("areg", "ut_p1")  # run again through MultiDISCO; AMPPI: "extended"


def fixture_name(s):
    return ("amppi_nav_" if s["kind"] == "amppi" else "skid_nav_") + s["tag"]


# ------------------------------------------------------------------------------------------------ maps
def map_cells(s):
    nx, ny = (int(math.ceil(d / s["cell"])) for d in s["map_dim"])  # ObstacleMap.__init__ (obstacle_map.py:21-24)
    return nx, ny


def make_map(s):
    """[nx, ny] float32 0 / 1 occupancy: BLOCK x BLOCK blocks occupied with probability p_occ; the start state's block is free"""
    nx, ny = map_cells(s)
    rng = np.random.default_rng(7000 + s["seed"])
    bx, by = -(-nx // BLOCK), -(-ny // BLOCK)
    m = np.kron((rng.random((bx, by)) < s["p_occ"]).astype(np.float32), np.ones((BLOCK, BLOCK), np.float32))[:nx, :ny]
    ix, iy = (int(math.floor(p / s["cell"] + n // 2)) for p, n in zip(s["state0"][:2], (nx, ny)))
    m[(ix // BLOCK) * BLOCK:(ix // BLOCK + 1) * BLOCK, (iy // BLOCK) * BLOCK:(iy // BLOCK + 1) * BLOCK] = 0.0
    return np.ascontiguousarray(m)


def pack_map(m):
    return np.packbits(np.asarray(m) != 0)


def unpack_map(g):
    nx, ny = (int(v) for v in g["map_shape"])
    return np.unpackbits(g["map_bits"])[:nx * ny].reshape(nx, ny).astype(np.float32)


def scaled64(xy, s, grid_shape):
    """p * (1 / cell) + centre in float64 (obstacle_map.py:78): [..., 2]"""
    return np.asarray(xy, np.float64) * (1 / s["cell"]) + np.array([int(grid_shape[0] / 2), int(grid_shape[1] / 2)], np.float64)


def scaled32(xy, s, grid_shape):
    """the same in fp32, operation by operation, as the reference's fp32 run and the device evaluate it"""
    return (np.asarray(xy, np.float32) * np.float32(1 / s["cell"]) + np.array([int(grid_shape[0] / 2), int(grid_shape[1] / 2)], np.float32)).astype(np.float32)


def occupancy(grid, sc, variant=None):
    """ObstacleMap.get_collisions (obstacle_map.py:64-93) of scaled positions sc [..., 2]: floor -> clamp -> gather, in float64.
    variant "round": round in place of floor; "transpose": the x and y index swapped; "free": off-map is free instead of clamped"""
    nx, ny = grid.shape
    idx = (np.round(sc) if variant == "round" else np.floor(sc)).astype(np.int64)
    ix, iy = idx[..., 0], idx[..., 1]
    if variant == "transpose":
        ix, iy = iy, ix
    inside = (ix >= 0) & (ix < nx) & (iy >= 0) & (iy < ny)
    occ = grid[np.clip(ix, 0, nx - 1), np.clip(iy, 0, ny - 1)].astype(np.float64)
    return occ * inside if variant == "free" else occ


def nav_terms(s, grid, states, variant=None):
    """(inst [..., H], term [...]) obstacle terms of rollouts states [..., H + 1, 5] as the controller of s["kind"] places them: MultiDISCO the
    instantaneous term on states 0 .. H - 1, AMPPI on 1 .. H, both the terminal one on state H.  variant: occupancy()'s, or "w0" (no
    term), "noterm" (no terminal term), "shift" (the instantaneous term where the OTHER controller has it)."""
    if variant == "w0":
        z = np.zeros(states.shape[:-2] + (states.shape[-2] - 1,))
        return z, z[..., 0]
    occ = s["w_obs"] * occupancy(grid, scaled64(states[..., 0:2], s, grid.shape), variant)
    first = (s["kind"] == "amppi") != (variant == "shift")  # instantaneous term on 1 .. H
    inst = occ[..., 1:] if first else occ[..., :-1]
    term = occ[..., -1] * (0.0 if variant == "noterm" else 1.0)
    return inst, term


def quad(x, w):
    return (((x - np.asarray(GOAL, np.float64)) ** 2) * np.asarray(w, np.float64)).sum(-1)


def weights(n, alpha):
    """float64 (loc_weights [2n + 1], lambda + n) of a Merwe scaled transform (utf.py:81-91), kappa = 0"""
    lam = alpha ** 2 * n - n
    w = np.full(2 * n + 1, 0.5 / (n + lam))
    w[0] = lam / (n + lam)
    return w, lam + n


def combine(s, inst, term, w=None):
    """per-rollout cost parts -> the controller's cost of a lane.  disco: inst [M, S, N, H], term [M, S, N] -> mean over M of (sum_t inst + term);
    ut: sum_m sum_t w[(m H + t) mod M] inst + sum_m w[m] term (disco.py:312-323); amppi: inst [S, pts, H], term [S, pts] -> weighted over pts"""
    if s["kind"] == "disco":
        return (inst.sum(-1) + term).mean(0)
    if s["kind"] == "ut":
        pts, H = inst.shape[0], inst.shape[-1]
        m, t = np.meshgrid(np.arange(pts), np.arange(H), indexing="ij")
        return np.einsum("msnt,mt->sn", inst, w[(m * H + t) % pts]) + np.einsum("msn,m->sn", term, w)
    if inst.shape[1] == 1:
        return term[:, 0] + inst.sum(-1)[:, 0]
    return term @ w + inst.sum(-1) @ w


def a_cov_of(s):
    return np.asarray(s["a_cov"] if s["a_cov"] is not None else ((SIGMA_A ** 2, 0.0), (0.0, SIGMA_A ** 2)), np.float64)


def dist_of(s):
    """(mean [P], std [P]) of the normal the sigma points / AMPPI's rows come from, fp32"""
    mean = np.array([s["fixed"][k] for k in s["up"]], np.float32)
    return mean, (np.float32(REL_STD) * mean).astype(np.float32)


def twin(g, q):
    """The float64 twin of a fixture's quantity q: stored whole as `q_f64`, or - the states - as `q_f64_delta32` (tests/ut_cases.py twin)"""
    if q + "_f64" in g:
        return g[q + "_f64"]
    return g[q].astype(np.float64) + g[q + "_f64_delta32"].astype(np.float64) / TWIN_SCALE


# ------------------------------------------------------------------------------------------------ inputs
def chol32(s):
    """L of the action covariance in fp32, as the library's configuration forms it: (L00, L10, L11)"""
    if s["a_cov"] is None:
        return np.float32(SIGMA_A), np.float32(0.0), np.float32(SIGMA_A)
    L = np.linalg.cholesky(np.asarray(s["a_cov"], np.float64))
    return np.float32(L[0, 0]), np.float32(L[1, 0]), np.float32(L[1, 1])


def actions_of(s, mean, eps):
    """mean + L eps in fp32, in the device's order of operations (skid.hpp, amppi.hpp)"""
    l00, l10, l11 = chol32(s)
    e0, e1 = eps[..., 0], eps[..., 1]
    a0 = mean[..., 0] + l00 * e0
    a1 = mean[..., 1] + ((l10 * e0 + l11 * e1) if l10 != 0 else l11 * e1)
    return np.stack([a0, a1], -1).astype(np.float32)


def inputs(s, seed):
    """the scenario's inputs from one seed of the generator's search"""
    rng = np.random.default_rng(seed)
    H = s["H"]
    inp = dict(state=np.array(s["state0"], np.float32))
    if s["kind"] == "amppi":
        S = s["S"]
        if s.get("a_seq0") == "edge":
            # the right wheel on the upper bound, the left one alternating between the bounds: forward on even steps, on the spot on odd ones
            a_seq0 = np.stack([np.full(H, s["bounds"][1]), np.where(np.arange(H) % 2 == 0, s["bounds"][1], s["bounds"][0])], 1).astype(np.float32)
        else:
            a_seq0 = (s["fwd"] + 0.4 * rng.standard_normal((H, 2))).astype(np.float32)
        eps = rng.standard_normal((S, H, 2)).astype(np.float32)
        inp.update(a_seq0=a_seq0, eps=eps, actions=actions_of(s, a_seq0[None], eps))
        if s["mode"] in ("single", "extended"):
            mean, std = dist_of(s)
            inp["params"] = (mean + std * rng.standard_normal((1 if s["mode"] == "single" else S, len(s["up"])))).astype(np.float32)
        if s["mode"] == "ut":
            inp["dist_mean"], inp["dist_std"] = dist_of(s)
        return inp
    N, S, M = s["N"], s["S"], s["M"]
    sign = np.where(np.arange(N) % 2 == 0, 1.0, -1.0)[:, None, None] if s.get("alternate") else 1.0
    a_mat0 = (sign * s["fwd"] + 0.5 * rng.standard_normal((N, H, 2))).astype(np.float32)
    eps = rng.standard_normal((S, N, H, 2)).astype(np.float32)
    a_seq0 = (0.5 * rng.standard_normal((H, 2)) if s["a_seq"] else np.zeros((H, 2))).astype(np.float32)
    inp.update(a_mat0=a_mat0, a_seq0=a_seq0, eps=eps, ext_actions=actions_of(s, a_mat0[None], eps))
    if s["kind"] == "ut":
        inp["dist_mean"], inp["dist_std"] = dist_of(s)
    elif s["up"]:
        P = len(s["up"])
        if s["dist"] == "uniform":
            p = rng.uniform(s["lo"], s["hi"], (M, P))
        else:
            p = np.asarray(s["loc"]) + np.asarray(s["scale"]) * rng.standard_normal((M, P))
        inp["params"] = p.astype(np.float32)
    return inp


def context_kwargs(s, **kw):
    """Context keywords of a scenario (without the map: Context(grid=unpack_map(g), ...))"""
    amppi = s["kind"] == "amppi"
    d = dict(model="skid_steer", N=1 if amppi else s["N"], S=s["S"], M=(2 * len(s["up"]) + 1 if s["mode"] == "ut" else 1) if amppi else s["M"], H=s["H"],
             dt=s["dt"], temperature=TEMPERATURE, alpha=1.0 / TEMPERATURE, ctrl_penalty=s["ctrl_penalty"], uncertain_params=s["up"] or None,
             params_log_space=s["log"], params_scalar_event=s["dist"] == "scalar", min_a=s["bounds"][0], max_a=s["bounds"][1], goal=GOAL,
             w_quad_state=W_STATE, w_quad_term=W_TERM, w_quad_ctrl=s["w_ctrl"], w_obs=s["w_obs"], cell_size=s["cell"], **s["fixed"])
    if amppi:
        d.update(a_cov=a_cov_of(s).astype(np.float32), sampling=s["mode"] != "none")
    else:
        d.update(sigma_a=SIGMA_A, sigma_p=SIGMA_A)
        if s["a_cov"] is not None:
            d["a_cov"] = np.asarray(s["a_cov"], np.float32)
    d.update(kw)
    return d


# ------------------------------------------------------------------------------------------------ float64 restatements
def rollouts64(s, state, acts, p, trig0=None):
    """SkidSteerRobot.step (skid_steer_robot.py:73-122) over acts [R, H, 2] from one start state, in float64; p: name -> float or [R, 1]
    column.  trig0: the (cos, sin) of the start heading the first step uses (MultiDISCO's float64 run keeps the start state in fp32,
    disco.py:369, and takes them from torch's fp32 routines - recorded in the fixture).  -> [R, H + 1, 5]"""
    R, H = acts.shape[0], acts.shape[1]
    x = np.tile(np.asarray(state, np.float32).astype(np.float64).reshape(1, 5), (R, 1))
    lo, hi = (float(np.float32(v)) for v in s["bounds"])  # (the action space holds its bounds in fp32: skid_steer_robot.py:51-53)
    traj = [x]
    for t in range(H):
        a = acts[:, t]
        r, l = np.clip(a[:, 0:1], lo, hi), np.clip(a[:, 1:2], lo, hi)
        lin = (r + l) * np.pi * p["wheel_radius"]
        ang = (r - l) * 2 * np.pi * p["wheel_radius"] / p["axial_distance"]
        fwd, lat = lin * s["dt"], -ang * p["x_icr"] * s["dt"]
        th = x[:, 2:3]
        cs, sn = np.cos(th), np.sin(th)
        if t == 0 and trig0 is not None:
            cs, sn = (float(v) for v in trig0)
        one = np.ones_like(th)
        x = np.concatenate([x[:, 0:1] + fwd * cs - lat * sn, x[:, 1:2] + fwd * sn + lat * cs, th + ang * s["dt"], lin * one, ang * one], 1)
        traj.append(x)
    return np.stack(traj, 1)


def restate_disco(s, g, grid):
    """MultiDISCO.forward with the navigation cost in float64 numpy from a fixture's fp32 inputs (kinds "disco" and "ut"): rollouts, costs
    (disco.py:294-346; the sigma-point form disco.py:211-292, 312-323), weights and the a_mat update (disco.py:380-393).
    -> dict of the ROLLOUT_QUANT arrays; states [M, S, N, H + 1, 5]"""
    N, S, H, M = s["N"], s["S"], s["H"], s["M"]
    f = lambda a: np.asarray(a, np.float64)
    p = {k: np.full((M * S * N, 1), v) for k, v in s["fixed"].items()}
    if s["kind"] == "ut":
        rows = np.repeat(f(g["sigma_points"]), S * N, 0)  # block m runs sigma point m
    elif s["up"]:
        raw = f(g["params"])
        raw = np.exp(raw) if s["log"] else raw
        if s["dist"] == "scalar":
            rows = np.tile(raw.reshape(1, -1), (1, S * N)).reshape(-1, 1)  # disco.py:177-179: rollout r takes params[r % M]
        else:
            rows = np.tile(raw.reshape(M, -1), (1, S * N)).reshape(-1, raw.reshape(M, -1).shape[1])
    for i, k in enumerate(s["up"]):
        p[k] = rows[:, i:i + 1]
    acts = f(g["ext_actions"])
    rep = np.tile(acts.reshape(-1, H, 2), (M, 1, 1))
    st = rollouts64(s, g["state"], rep, p, g["trig0_f32"]).reshape(M, S, N, H + 1, 5)
    ni, nt = nav_terms(s, grid, st)
    ctrl = ((acts ** 2) * f(s["w_ctrl"])).sum(-1)[None]  # [1, S, N, H]
    inst = quad(st[..., :-1, :], W_STATE) + ctrl + ni
    term = quad(st[..., -1, :], W_TERM) + nt
    costs = combine(s, inst, term, weights(len(s["up"]), float(g["alpha"]))[0] if s["kind"] == "ut" else None)
    a_mat, a_seq = f(g["a_mat0"]), f(g["a_seq0"])
    eps = acts - a_seq
    a_reg = TEMPERATURE * (1 - s["ctrl_penalty"])
    costs = costs + a_reg * np.einsum("snhd,nhd->sn", -eps, a_mat @ np.linalg.inv(a_cov_of(s)))
    lc = -1 * (costs - costs.min()) / TEMPERATURE
    mx = lc.max(0)
    eta = mx + np.log(np.exp(lc - mx).sum(0))
    omega = np.exp(lc - eta)
    return dict(costs=costs, states=st, omega=omega, a_mat1=a_mat + np.einsum("sn,snhd->nhd", omega, eps),
                a_mix=np.exp(eta - (eta.max() + np.log(np.exp(eta - eta.max()).sum()))))


def restate_amppi(s, g, grid):
    """AMPPI.update_actions (amppi.py:193-260) with the navigation cost in float64 numpy from a fixture's fp32 inputs
    -> dict(costs [S], omega [S], a_seq1 [H, 2], states [S pts, H + 1, 5])"""
    S, H = s["S"], s["H"]
    f = lambda a: np.asarray(a, np.float64)
    a_seq, acts = f(g["a_seq0"]), f(g["actions"])
    eps = acts - a_seq[None]
    pts = 2 * len(s["up"]) + 1 if s["mode"] == "ut" else 1
    p = dict(s["fixed"])
    if s["mode"] == "ut":
        rows = np.tile(f(g["sigma_points"]), (S, 1))  # trajectory s * pts + k runs point k
    elif s["mode"] == "single":
        rows = np.repeat(f(g["params"])[:1], S, 0)
    elif s["mode"] == "extended":
        rows = f(g["params"])
    for i, k in enumerate(s["up"] if s["mode"] != "none" else ()):
        p[k] = rows[:, i:i + 1]
    st = rollouts64(s, g["state"], np.repeat(acts, pts, 0), p)
    ni, nt = nav_terms(s, grid, st)
    inst = (quad(st[:, 1:], W_STATE) + ni).reshape(S, pts, H)
    term = (quad(st[:, -1], W_TERM) + nt).reshape(S, pts)
    lam = TEMPERATURE
    costs = combine(s, inst, term, weights(len(s["up"]), s["alpha"])[0] if pts > 1 else None)
    costs = costs + lam * np.einsum("td,std->s", a_seq @ np.linalg.inv(a_cov_of(s).astype(np.float32).astype(np.float64)), eps)
    lc = (-1 / lam) * (costs - costs.min())
    omega = lc - (lc.max() + np.log(np.exp(lc - lc.max()).sum()))
    lo, hi = (float(np.float32(v)) for v in s["bounds"])
    return dict(costs=costs, omega=omega, a_seq1=np.clip(a_seq + np.tensordot(np.exp(omega), eps, 1), lo, hi), states=st)


def costs_off(s, g, grid, variant):
    """The fixture's fp32 costs with the obstacle terms of `variant` in place of the true ones, from the fixture's own fp32 states (exact:
    the terms are w_obs times 0 / 1, the edge margin keeps every cell) - fp32"""
    st = g["states"].astype(np.float64)
    w = None
    if s["kind"] == "amppi":
        pts = st.shape[0] // s["S"]
        shape = lambda it: (it[0].reshape(s["S"], pts, -1), it[1].reshape(s["S"], pts))
        w = weights(len(s["up"]), s["alpha"])[0] if pts > 1 else None
    else:
        shape = lambda it: it
        w = weights(len(s["up"]), float(g["alpha"]))[0] if s["kind"] == "ut" else None
    on = combine(s, *shape(nav_terms(s, grid, st)), w)
    off = combine(s, *shape(nav_terms(s, grid, st, variant)), w)
    return (g["costs"].astype(np.float64) + (off - on)).astype(np.float32)
