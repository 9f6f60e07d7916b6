"""Sigma-point ("DISCO" case) test scenarios of the skid-steer and cart-pole families and of the filter's sigma points (TEST
INFRASTRUCTURE), shared by tests/golden/make_golden_ut_families.py, which runs the reference on them, and by the tests that read the
resulting tests/golden/ut_*.npz.  Data and seeded numpy only: nothing here imports the reference or the library.

Rollout scenarios (ROLLOUTS) are dicts: tag, family ("cartpole" / "skid"), N, S, H, up (uncertain parameter names in column order: P
of them, 2P + 1 sigma points), seed, states (store every rollout's states), mean (store the plain-mean costs too).  The parameter
distribution is a MultivariateNormal around the constructor defaults with REL_STD standard deviations.  N S = 300 lanes: one full
256-lane block and a ragged second one; H = 7 is coprime with 3, 5 and 9 sigma points, so the (sigma, step) weight pattern of
disco.py:314-316 shifts from rollout to rollout - and equals the 7 points of the skid-steer P = 3 case, where H is a multiple of M.
The instantaneous cost is action-free (the reference hands its cost function S N pts H states and S N H actions, disco.py:306-309).
Filter scenarios (SIGMA_MPF): tag, Mp, P, bw, spread, seed - particles of unit scale; SIGMA_UP names the uncertain parameters a filter of each
family is built with to carry them (the sigma points depend on the particles and the bandwidth only).
"""
import numpy as np

import cartpole_cases as cp
import mpf_skid_cases as sk

ALPHA, REL_STD, CAP, TOL = 0.5, 0.1, 5e-5, 1e-5

# the skid-steer controller scenarios: the quadratic cost, start state and noise scale of the family's earlier fixtures (skid_*.npz); the
# temperature is 4 instead of their 0.8: costs near 40 over 0.8 put the reference's own fp32 omega 6e-5 from its float64 one, over the cap
SKID = dict(goal=(1.0, 0.5, 0.3, 0.0, 0.0), w_state=(2.0, 2.0, 0.5, 0.1, 0.05), w_term=(50.0, 50.0, 5.0, 0.0, 0.0), w_ctrl=(0.0, 0.0),
            state0=(0.3, -0.2, 0.4, 0.1, -0.05), sigma_a=0.3, a_scale=0.25, temperature=4.0, dt=0.1, lo=(-0.5, -0.5), hi=(0.5, 0.5),
            defaults=sk.DEFAULTS, ds=5, da=2)
# the cart-pole scenarios: the family's quadratic cost, start state and noise scale (cartpole_cases.py), but temperature 0.25 instead of 4:
# omega and a_mix are held to the amplification of eight cost ulps through exp(-cost / temperature), 8 ulp(max cost) / temperature, and
# that bound models the rounding of the COSTS only.  With these costs of 1 ... 3 over a temperature of 4 it is 2.4e-7, below the fp32
# rounding of the softmax itself (the reference's own fp32 omega is 4.6e-7 ... 6.8e-7 from its float64 omega there, measured by the
# generator): no fp32 implementation can be asked for it.  At cost / temperature near 10, as in the skid-steer scenarios, the costs'
# rounding is what the weights carry and the bound says something.
CART = dict(goal=cp.GOAL, w_state=cp.W_STATE, w_term=cp.W_TERM, w_ctrl=(0.0,), state0=cp.STATE0, sigma_a=cp.SIGMA_A, a_scale=0.5,
            temperature=0.25, dt=cp.DT, defaults=cp.DEFAULTS, ds=4, da=1)
FAMILY = dict(skid=SKID, cartpole=CART)


def R(tag, family, up, seed, N=5, S=60, H=7, states=False, mean=False, **kw):
    return dict(tag=tag, family=family, up=tuple(up), seed=seed, N=N, S=S, H=H, states=states, mean=mean, **kw)


ROLLOUTS = [
    R("cartpole_p1", "cartpole", ("length",), 61),
    R("cartpole_p2", "cartpole", ("mass_pole", "length"), 62, states=True, mean=True),
    R("cartpole_p4", "cartpole", ("length", "g", "mass_pole", "mass_cart"), 63),  # (a non-canonical column order)
    R("skid_p1", "skid", ("axial_distance",), 71),
    R("skid_p2", "skid", ("wheel_radius", "x_icr"), 72, states=True, mean=True),
    R("skid_p3", "skid", ("x_icr", "wheel_radius", "axial_distance"), 73),  # H = 7 = pts: the weight index is t for every sigma point
]
ROLLOUT_NAMES = [s["tag"] for s in ROLLOUTS]
ROLLOUT_BY_TAG = {s["tag"]: s for s in ROLLOUTS}
ROLLOUT_QUANT = ("costs", "states", "omega", "a_mat1", "a_mix")

# whole SVMPC ticks (K1, SGD, cartpole_cases.TICK_ITERS iterations, then forward) over a sigma-point controller
TICKS = [
    R("cartpole_tick", "cartpole", ("mass_pole", "length"), 81, N=8, S=16, H=12, lr=0.05, alpha=0.25),
    R("skid_tick", "skid", ("wheel_radius", "x_icr"), 82, N=8, S=16, H=12, lr=0.05, alpha=0.5),
]
TICK_NAMES = [s["tag"] for s in TICKS]
TICK_BY_TAG = {s["tag"]: s for s in TICKS}


def weights(n, alpha=ALPHA, beta=2.0, kappa=0.0):
    """float64 (loc_weights [2n + 1], lambda + n) of a Merwe scaled transform (utf.py:81-91)"""
    lam = alpha ** 2 * (n + kappa) - n
    w = np.full(2 * n + 1, 0.5 / (n + lam))
    w[0] = lam / (n + lam)
    return w, lam + n


def dist_of(s):
    """(mean [P], std [P]) of the scenario's parameter distribution, fp32"""
    d = FAMILY[s["family"]]["defaults"]
    mean = np.array([d[k] for k in s["up"]], np.float32)
    return mean, (np.float32(REL_STD) * mean).astype(np.float32)


def ut_costs(states, w, goal, w_state, w_term, shifted=True):
    """The weighted costs of disco.py:312-323 in float64 numpy from states [pts, S, N, H + 1, ds]:
    sum_m sum_t w[(m H + t) mod pts] inst(x_mt) + sum_m w[m] term(x_mH); shifted=False weights the instantaneous part by w[m]."""
    states = np.asarray(states, np.float64)
    pts, H = states.shape[0], states.shape[3] - 1
    d2 = (states - np.asarray(goal, np.float64)) ** 2
    inst = (d2[..., :-1, :] * np.asarray(w_state, np.float64)).sum(-1)  # [pts, S, N, H]
    term = (d2[..., -1, :] * np.asarray(w_term, np.float64)).sum(-1)    # [pts, S, N]
    m, t = np.meshgrid(np.arange(pts), np.arange(H), indexing="ij")
    wi = np.asarray(w, np.float64)[(m * H + t) % pts if shifted else m]  # [pts, H]
    return np.einsum("msnt,mt->sn", inst, wi) + np.einsum("msn,m->sn", term, np.asarray(w, np.float64))


def twin(g, q):
    """The float64 twin of a fixture's quantity q: stored whole as `q_f64`, or - the rollouts' states - as `q_f64_delta32`, its difference
    from the fp32 value, taken in float64, times cartpole_cases.TWIN_SCALE, in fp32 (the twin comes back to 1e-14 of a state)."""
    if q + "_f64" in g:
        return g[q + "_f64"]
    return g[q].astype(np.float64) + g[q + "_f64_delta32"].astype(np.float64) / cp.TWIN_SCALE


def context_kwargs(s, **kw):
    """Context keywords of a controller scenario (M = the sigma points)"""
    f = FAMILY[s["family"]]
    d = dict(N=s["N"], S=s["S"], M=2 * len(s["up"]) + 1, H=s["H"], dt=f["dt"], sigma_a=f["sigma_a"], sigma_p=f["sigma_a"],
             temperature=f["temperature"], alpha=1.0 / f["temperature"], uncertain_params=s["up"], goal=f["goal"], w_quad_state=f["w_state"],
             w_quad_term=f["w_term"], w_quad_ctrl=f["w_ctrl"])
    if s["family"] == "cartpole":
        d.update(model="cartpole", **f["defaults"])
    else:
        d.update(model="skid_steer")
    d.update(kw)
    return d


# ------------------------------------------------------------------------------------------------ the filter's sigma points
SIGMA_SIZES = (1, 2, 63, 64, 257, 1024)
SIGMA_UP = {("cartpole", 1): ("length",), ("cartpole", 4): ("g", "length", "mass_pole", "mass_cart"),
            ("skid", 1): ("axial_distance",), ("pendulum", 1): ("length",)}


def F(Mp, P, seed):
    """particles of unit scale (the kernel sees numbers, not a model): spread 0.15 around (1.0, 0.8, 1.3, 0.6), bandwidth 0.1 - of the
    order of the spread, so that leaving bw^2 out of the variance moves the points by far more than a tolerance"""
    return dict(tag="%d_p%d" % (Mp, P), Mp=Mp, P=P, bw=0.1, spread=0.15, seed=seed)


SIGMA_MPF = [F(Mp, P, 900 + 10 * i + P) for i, Mp in enumerate(SIGMA_SIZES) for P in (1, 4)]
SIGMA_NAMES = [s["tag"] for s in SIGMA_MPF]
SIGMA_BY_TAG = {s["tag"]: s for s in SIGMA_MPF}
SIGMA_CENTRE = (1.0, 0.8, 1.3, 0.6)


def sigma_particles(s):
    rng = np.random.default_rng(s["seed"])
    c = np.asarray(SIGMA_CENTRE[:s["P"]])
    return (c * np.exp(s["spread"] * rng.standard_normal((s["Mp"], s["P"])))).astype(np.float32)
