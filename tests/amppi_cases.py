"""AMPPI test scenarios (TEST INFRASTRUCTURE), shared by tests/golden/make_golden_amppi.py, which runs the reference's
`AMPPI.update_actions` (dust/controllers/amppi.py:227-260) on them, and by the tests that read the resulting tests/golden/amppi_*.npz.
Data and seeded numpy only: nothing here imports the reference or the library.

A scenario is a dict: tag, family ("pendulum" / "cartpole" / "skid" / "particle"), S, H, mode ("none" / "single" / "extended" / "ut"),
up (uncertain parameter names in column order), seed, states (keep every trajectory's states), and optionally a_cov (a full 2 x 2
action covariance), a_seq0 ("edge": the start sequence sits ON the action bounds, alternating, so that the final clamp acts), ticks (the
closed loop of `pend_loop`).  Operating points per family (FAMILY): lambda, noise scale, start state, cost - chosen so that, with the
reference alone, the largest weight e^omega stays <= 0.5, the update moves a_seq by >= 100 tolerances and every tolerance stays under the
cap (the generator asserts all three).

`restate` is section 1 of the AMPPI issue in float64 numpy - noise, steps, costs on states 1 .. H, sigma-point weights, the lambda
term, softmax, clamp - and `variant=` leaves one thing out (the fixtures' power variants).  The generator asserts that it reproduces the
reference's float64 run, the CPU tests that it reproduces each fixture's float64 twin.
"""
import math

import numpy as np

import cartpole_cases as cp
import mpf_skid_cases as sk
import ut_cases as ut

CAP, TOL = 5e-5, 1e-5
UT_ALPHA = 0.5  # MerweScaledUTF(alpha=): weights (1 - 1 / alpha^2, 1 / (2 n alpha^2), ...)
REL_STD = 0.1   # standard deviation of every uncertain parameter, relative to its default

PEND = dict(model="pendulum", ds=2, da=1, lam=100.0, sigma_a=2.0, a_scale=0.5, state0=(3.0, 0.0), dt=0.05, lo=(-2.0,), hi=(2.0,),
            defaults=dict(g=9.8, mass=1.0, length=1.0), w_cos=50.0, w_vel=1.0, max_speed=8.0)
CART = dict(model="cartpole", ds=4, da=1, lam=1.0, sigma_a=cp.SIGMA_A, a_scale=0.15, state0=cp.STATE0, dt=cp.DT, lo=(-1.0,), hi=(1.0,),
            defaults=cp.DEFAULTS, goal=cp.GOAL, w_state=cp.W_STATE, w_term=cp.W_TERM)
SKID = dict(model="skid_steer", ds=5, da=2, lam=4.0, sigma_a=ut.SKID["sigma_a"], a_scale=ut.SKID["a_scale"], state0=ut.SKID["state0"],
            dt=ut.SKID["dt"], lo=ut.SKID["lo"], hi=ut.SKID["hi"], defaults=sk.DEFAULTS, goal=ut.SKID["goal"], w_state=ut.SKID["w_state"],
            w_term=ut.SKID["w_term"])
# Particle as the demo configures it (demo/particle_config.yaml:39-61): grid_4x4 obstacles of width 2.1 on a 22 x 22 map of 0.1 cells,
# crashes on; the start state heads into the obstacle at (-2, -6) .. so that part of the trajectories crash within the horizon
# (the demo's cost weights put 1e6 on a crash and 1e3 on the final distance: costs of 1e6 leave fp32 no digits for the weights.  These keep
# every term - distance, speed, crash - within two orders of each other, so that a wrong one shows)
PART_COST = dict(w_qpos=0.01, w_qvel=1.0, w_ctrl=0.2, w_obs=20.0, w_qpos_T=0.1, w_qvel_T=1.0)
PART = dict(model="particle", ds=4, da=2, lam=50.0, sigma_a=5.0, a_scale=0.5, state0=(-3.3, -7.3, 4.0, 3.0), dt=0.015, lo=(-10.0, -10.0),
            hi=(10.0, 10.0), defaults=dict(mass=2.0), target=(9.0, 9.0, 0.0, 0.0), w_state=(0.01, 0.01, 1.0, 1.0), w_term=(0.1, 0.1, 1.0, 1.0),
            w_ctrl=(0.2, 0.2), w_obs=20.0, max_speed=5.0, max_accel=10.0, cell=0.1, cost_params=PART_COST)
# Particle(**PART_ENV, mass=, uncertain_params=): the constructor keywords of the scenario's model, for the reference's class and the repo's
PART_ENV = dict(dt=0.015, control_type="acceleration", noise_std=[0.1, 0.1], init_state=list(PART["state0"]), target_state=list(PART["target"]),
                can_crash=True, with_obstacle=True, deterministic=True, cost_params=PART_COST, obst_preset="grid_4x4", obst_width=2.1, max_speed=5,
                max_accel=10, map_cell_size=0.1, map_size=[22, 22], map_type="direct")
FAMILY = dict(pendulum=PEND, cartpole=CART, skid=SKID, particle=PART)


def A(tag, family, S, H, mode, up, seed, states=False, **kw):
    return dict(tag=tag, family=family, S=S, H=H, mode=mode, up=tuple(up), seed=seed, states=states, **kw)


SCENARIOS = [
    A("pend_one", "pendulum", 1, 1, "none", (), 101, states=True),
    A("pend_single_64", "pendulum", 64, 8, "single", ("length",), 102, states=True),
    A("pend_ext_257", "pendulum", 257, 31, "extended", ("length",), 103),
    A("pend_ext2_1021", "pendulum", 1021, 30, "extended", ("mass", "length"), 104),
    A("pend_ut_65", "pendulum", 65, 8, "ut", ("length",), 105, states=True),
    A("pend_big_4099", "pendulum", 4099, 12, "extended", ("length",), 106),
    A("pend_clamp", "pendulum", 64, 8, "none", (), 108, a_seq0="edge"),  # (seed 107: top weight 0.68)
    A("cart_none_64", "cartpole", 64, 8, "none", (), 111, states=True),
    A("cart_ext_255", "cartpole", 255, 12, "extended", ("mass_pole", "length"), 112),
    A("cart_ut_64", "cartpole", 64, 8, "ut", ("mass_pole", "length"), 113, states=True),
    A("skid_none_63", "skid", 63, 8, "none", (), 121, a_cov=((0.09, 0.03), (0.03, 0.0625))),
    A("skid_ext_256", "skid", 256, 10, "extended", ("x_icr", "wheel_radius", "axial_distance"), 122),
    A("skid_ut_33", "skid", 33, 8, "ut", ("x_icr", "wheel_radius", "axial_distance"), 124, states=True),  # (seed 123: top weight 0.65)
    A("part_none_64", "particle", 64, 10, "none", (), 131, states=True),
    A("part_ext_257", "particle", 257, 10, "extended", ("mass",), 132),
]
LOOP = A("pend_loop", "pendulum", 64, 8, "extended", ("length",), 141, ticks=4)
NAMES = [s["tag"] for s in SCENARIOS]
BY_TAG = {s["tag"]: s for s in SCENARIOS + [LOOP]}
QUANT = ("costs", "omega", "a_seq1")
CLASS_CASES = ("pend_ext_257", "cart_ut_64", "skid_none_63", "part_none_64")  # run again through the AMPPI class


def weights(n):
    return ut.weights(n, UT_ALPHA)


def a_cov_of(s):
    """[da, da] fp32 action covariance"""
    f = FAMILY[s["family"]]
    return np.asarray(s["a_cov"], np.float32) if "a_cov" in s else (np.float32(f["sigma_a"]) ** 2 * np.eye(f["da"], dtype=np.float32))


def dist_of(s):
    """(mean [P], std [P]) of the scenario's parameter distribution, fp32"""
    d = FAMILY[s["family"]]["defaults"]
    mean = np.array([d[k] for k in s["up"]], np.float32)
    return mean, (np.float32(REL_STD) * mean).astype(np.float32)


def draw_actions(s, rng, a_seq):
    """[S, H, da] fp32 actions around a_seq: a_seq + L z with L = cholesky(a_cov)"""
    f = FAMILY[s["family"]]
    L = np.linalg.cholesky(a_cov_of(s).astype(np.float64)).astype(np.float32)
    z = rng.standard_normal((s["S"], s["H"], f["da"])).astype(np.float32)
    return (a_seq[None] + z @ L.T).astype(np.float32)


def draw_params(s, rng):
    """the recorded rows model.sample_params hands out: [1, P] ("single"), [S, P] ("extended"), else None"""
    if s["mode"] not in ("single", "extended"):
        return None
    mean, std = dist_of(s)
    n = 1 if s["mode"] == "single" else s["S"]
    return (mean + std * rng.standard_normal((n, len(s["up"])))).astype(np.float32)


def inputs(s):
    f = FAMILY[s["family"]]
    rng = np.random.default_rng(s["seed"])
    H, da = s["H"], f["da"]
    if s.get("a_seq0") == "edge":
        a_seq0 = (np.asarray(f["hi"], np.float32) * np.where(np.arange(H) % 2 == 0, 1.0, -1.0)[:, None]).astype(np.float32)
    else:
        a_seq0 = (f["a_scale"] * rng.standard_normal((H, da))).astype(np.float32)
    inp = dict(state=np.array(f["state0"], np.float32), a_seq0=a_seq0, actions=draw_actions(s, rng, a_seq0))
    p = draw_params(s, rng)
    if p is not None:
        inp["params"] = p
    if s["mode"] == "ut":
        inp["dist_mean"], inp["dist_std"] = dist_of(s)
    return inp


def loop_inputs(s):
    """the closed loop: per tick the recorded standard-normal draws (the actions are a_seq + sigma_a z around the CURRENT sequence) and
    parameter rows"""
    f = FAMILY[s["family"]]
    rng = np.random.default_rng(s["seed"])
    T, S, H, da = s["ticks"], s["S"], s["H"], f["da"]
    mean, std = dist_of(s)
    return dict(state=np.array(f["state0"], np.float32), a_seq0=(f["a_scale"] * rng.standard_normal((H, da))).astype(np.float32),
                z=rng.standard_normal((T, S, H, da)).astype(np.float32),
                params=(mean + std * rng.standard_normal((T, S, len(s["up"])))).astype(np.float32))


def context_kwargs(s, **kw):
    """Context keywords of a scenario (N = 1: an AMPPI context)"""
    f = FAMILY[s["family"]]
    sampled = s["mode"] != "none"
    d = dict(model=f["model"], N=1, S=s["S"], M=2 * len(s["up"]) + 1 if s["mode"] == "ut" else 1, H=s["H"], dt=f["dt"], temperature=f["lam"],
             alpha=1.0 / f["lam"], a_cov=a_cov_of(s), min_a=f["lo"], max_a=f["hi"], uncertain_params=s["up"] or None, sampling=sampled)
    if s["family"] == "pendulum":
        d.update(w_cos=f["w_cos"], w_vel=f["w_vel"], **f["defaults"])
    elif s["family"] == "particle":
        d.update(mass=f["defaults"]["mass"], target=f["target"], w_state=f["w_state"], w_term=f["w_term"], w_ctrl=f["w_ctrl"], w_obs=f["w_obs"],
                 max_speed=f["max_speed"], max_accel=f["max_accel"], can_crash=True, with_obstacle=True, cell_size=f["cell"], deterministic=True)
    else:
        d.update(goal=f["goal"], w_quad_state=f["w_state"], w_quad_term=f["w_term"], w_quad_ctrl=(0.0,) * f["da"], **f["defaults"])
    d.update(kw)
    return d


def twin(g, q):
    """float64 twin of quantity q: stored whole, or (states) as its scaled difference from the fp32 value in fp32"""
    if q + "_f64" in g:
        return g[q + "_f64"]
    return g[q].astype(np.float64) + g[q + "_f64_delta32"].astype(np.float64) / cp.TWIN_SCALE


# ------------------------------------------------------------------------------------------------ float64 restatement
def _collisions(grid, xy, cell):
    """ObstacleMap.get_collisions (obstacle_map.py:64-93): floor(x / cell + centre) -> clamp -> gather"""
    nx, ny = grid.shape
    occ = np.floor(xy * (1 / cell) + np.array([int(nx / 2), int(ny / 2)], np.float64)).astype(np.int64)
    return grid[np.clip(occ[:, 0], 0, nx - 1), np.clip(occ[:, 1], 0, ny - 1)].astype(np.float64)


def _step(s, x, a, p, grid):
    """one model step in float64: x [n, ds], a [n, da], p: name -> Python float or [n, 1] column"""
    fam, f = s["family"], FAMILY[s["family"]]
    dt = f["dt"]
    if fam == "pendulum":  # pendulum.py:82-100
        th, thd = x[:, :1], x[:, 1:]
        g, m, ln = p["g"], p["mass"], p["length"]
        u = np.clip(a, f["lo"][0], f["hi"][0])
        # (a Python float over a tensor is reciprocal() * float in torch: it matters where the sigma points keep the quotient in fp32)
        thd = thd + dt * ((1.0 / (2 * ln)) * (-3 * g) * np.sin(th + math.pi) + (1.0 / (m * ln ** 2)) * 3.0 * u)
        thd = np.clip(thd, -f["max_speed"], f["max_speed"])
        return np.concatenate((th + thd * dt, thd), 1)
    if fam == "cartpole":  # cartpole.py:148-172
        g, m_c, m_p, ln, mu_c, mu_p, f_mag = (p[k] for k in cp.NAMES7)
        x_d, th, th_d = x[:, 1:2], x[:, 2:3], x[:, 3:4]
        u = np.clip(a, -1, 1) * f_mag
        mass, pm = m_c + m_c, m_p * ln
        fac = (u + pm * np.sin(th) * th_d ** 2 - mu_c * np.sign(x_d)) / mass
        num = g * np.sin(th) - np.cos(th) * fac - (mu_p * th_d) / pm
        den = ln * (4.0 / 3 - (m_p * np.cos(th) ** 2) / mass)
        th_dd = num / den
        x_dd = fac - pm * th_dd * np.cos(th) / mass
        return x + np.concatenate((x_d, x_dd, th_d, th_dd), 1) * dt
    if fam == "skid":  # skid_steer_robot.py:84-122
        xicr, wr, ad = p["x_icr"], p["wheel_radius"], p["axial_distance"]
        r, l = np.clip(a[:, :1], f["lo"][0], f["hi"][0]), np.clip(a[:, 1:], f["lo"][1], f["hi"][1])
        lin = (r + l) * math.pi * wr
        ang = (r - l) * 2 * math.pi * wr / ad
        fwd, lat = lin * dt, -ang * xicr * dt
        th = x[:, 2:3]
        one = np.ones_like(th)
        return np.concatenate((x[:, :1] + fwd * np.cos(th) - lat * np.sin(th), x[:, 1:2] + fwd * np.sin(th) + lat * np.cos(th), th + ang * dt,
                               lin * one, ang * one), 1)
    # particle.py:135-166, acceleration control, deterministic, can_crash with obstacles
    acc = np.clip(a / p["mass"], -f["max_accel"], f["max_accel"])
    xd = np.concatenate((x[:, 2:], acc), 1)
    nxt = x + xd * dt * (1 - _collisions(grid, x[:, :2], f["cell"])[:, None])
    nxt[:, 2:] = np.clip(nxt[:, 2:], -f["max_speed"], f["max_speed"])
    return nxt


def _costs(s, x, grid, term):
    """instantaneous (no action) or terminal cost of states x [n, ds]"""
    fam, f = s["family"], FAMILY[s["family"]]
    if fam == "pendulum":  # demo/pendulum_example.py:21-28
        return f["w_cos"] * (np.cos(x[:, 0]) - 1) ** 2 + f["w_vel"] * x[:, 1] ** 2
    if fam == "particle":  # particle.py:170-225 with actions = 0
        w = np.asarray(f["w_term" if term else "w_state"], np.float64)
        d = x - np.asarray(f["target"], np.float64)
        return (d * d * w).sum(-1) + f["w_obs"] * _collisions(grid, x[:, :2], f["cell"])
    w = np.asarray(f["w_term" if term else "w_state"], np.float64)
    return (((x - np.asarray(f["goal"], np.float64)) ** 2) * w).sum(-1)


def restate(s, inp, variant=None, grid=None, sigma_points=None):
    """-> dict(costs [S], omega [S], a_seq1 [H, da], states [S pts, H + 1, ds]) in float64 from the fp32 inputs.
    variant: "disco" (instantaneous cost on t = 0 .. H - 1), "noctrl" (no lambda term), "single" (row 0 for every trajectory),
    "mean" (plain mean over the sigma points), "noclamp" (no final clamp)."""
    f = FAMILY[s["family"]]
    S, H, da, ds, lam = s["S"], s["H"], f["da"], f["ds"], f["lam"]
    a_seq = inp["a_seq0"].astype(np.float64)
    acts = inp["actions"].astype(np.float64)
    eps = acts - a_seq[None]
    pts = 2 * len(s["up"]) + 1 if s["mode"] == "ut" else 1
    p = dict(f["defaults"])
    if s["mode"] == "ut":
        # trajectory s * pts + k runs point k.  The points stay fp32 (utf.py:108-118 casts them) while the states are float64: products of
        # parameters alone round to fp32 before they meet a state, as the reference's own float64 run has it
        rows = np.tile(np.asarray(sigma_points, np.float32), (S, 1))
    elif s["mode"] in ("single", "extended"):
        rows = inp["params"].astype(np.float64)
        if s["mode"] == "single" or variant == "single":
            rows = np.repeat(rows[:1], S, 0)
    if s["mode"] != "none":
        for i, k in enumerate(s["up"]):
            p[k] = rows[:, i:i + 1]
    x = np.repeat(np.asarray(inp["state"], np.float32).astype(np.float64)[None], S * pts, 0)  # (amppi.py:244 casts the state to fp32)
    a_rep = np.repeat(acts, pts, 0)  # [S pts, H, da]
    traj = [x]
    for t in range(H):
        x = _step(s, x, a_rep[:, t], p, grid)
        traj.append(x)
    traj = np.stack(traj, 1)  # [S pts, H + 1, ds]
    sl = traj[:, :-1] if variant == "disco" else traj[:, 1:]
    inst = _costs(s, sl.reshape(-1, ds), grid, False).reshape(S * pts, H).sum(1)
    term = _costs(s, traj[:, -1], grid, True)
    if pts > 1:
        w = np.full(pts, 1.0 / pts) if variant == "mean" else weights(len(s["up"]))[0]
        inst, term = inst.reshape(S, pts) @ w, term.reshape(S, pts) @ w
    pre = np.linalg.inv(a_cov_of(s).astype(np.float64))
    ctrl = lam * np.einsum("td,std->s", a_seq @ pre, eps)
    costs = term + inst + (0.0 if variant == "noctrl" else ctrl)
    lc = (-1 / lam) * (costs - costs.min())
    omega = lc - (lc.max() + np.log(np.exp(lc - lc.max()).sum()))
    a1 = a_seq + np.tensordot(np.exp(omega), eps, 1)
    if variant != "noclamp":
        a1 = np.clip(a1, np.asarray(f["lo"], np.float64), np.asarray(f["hi"], np.float64))
    return dict(costs=costs, omega=omega, a_seq1=a1, states=traj)


def restate_loop(s, inp):
    """the closed loop of `pend_loop` in float64: per tick restate() from the recorded actions and rows, the plant's step on the nominal
    model with the first planned action, roll(1) -> dict(costs [T, S], omega [T, S], a_seq1 [T, H, da], plant [T, ds])"""
    f = FAMILY[s["family"]]
    nominal = dict(s, mode="none", up=())
    a_seq, state = inp["a_seq0"].astype(np.float64), inp["state"].astype(np.float64)
    out = {k: [] for k in QUANT + ("plant",)}
    for k in range(s["ticks"]):
        r = restate(s, dict(state=state, a_seq0=a_seq, actions=inp["actions"][k], params=inp["params"][k]))
        state = _step(nominal, state[None], r["a_seq1"][:1], dict(f["defaults"]), None)[0]
        a_seq = np.concatenate((r["a_seq1"][1:], np.zeros((1, f["da"]))), 0)
        for q in QUANT:
            out[q].append(r[q])
        out["plant"].append(state)
    return {k: np.stack(v) for k, v in out.items()}


LOOP_VARIANTS = ("disco", "noctrl", "single")


def restate_loop_variants(s, inp, a_seq1, plant):
    """the loop's power variants: per tick the costs with one thing left out, from the TRUE loop's inputs of that tick (the float64
    sequence and plant state the tick started from) -> dict(costs_<variant> [T, S])"""
    f = FAMILY[s["family"]]
    a_seq, state = inp["a_seq0"].astype(np.float64), inp["state"].astype(np.float64)
    out = {v: [] for v in LOOP_VARIANTS}
    for k in range(s["ticks"]):
        tick = dict(state=state, a_seq0=a_seq, actions=inp["actions"][k], params=inp["params"][k])
        for v in LOOP_VARIANTS:
            out[v].append(restate(s, tick, variant=v)["costs"])
        state = np.asarray(plant[k], np.float64)
        a_seq = np.concatenate((np.asarray(a_seq1[k], np.float64)[1:], np.zeros((1, f["da"]))), 0)
    return {"costs_" + v: np.stack(c) for v, c in out.items()}
