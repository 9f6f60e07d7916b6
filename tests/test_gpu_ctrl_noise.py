"""Device-drawn control noise of a noisy Particle (Particle(deterministic=False), noise_std != 0: every step drives the dynamics with
action + noise_std z, particle.py:145-148) pinned ELEMENT-WISE against the CPU oracle.

The draws come from three Philox layouts (tests/philox_ref.py states them): rollout.hpp's packed pair path (lean kernel), its
one-sample loop (the rollouts the pairs leave over; every rollout of the full kernel) and particle_general.hpp's Philox branch (stored
states, velocity control).  The device's own normals at the replica's counters (dust_debug_philox: the hardware transcendentals differ
from float64 Box-Muller by ~1e-6, which must not reach a rollout next to an obstacle) are assembled into Z [H][M*S*N][2] and handed to
Oracle.rollout_cost(..., ctrl_noise=Z) and, through set_ctrl_noise, to a twin context's recorded-draw path (the one the goldens pin)."""
import ctypes as C

import numpy as np
import pytest

import philox_ref as pr
from helpers import elemerr, relerr

pytestmark = pytest.mark.gpu
TOL = 1e-5
SEED = 0x00C0FFEE0000002A  # (a high key word: the control keys XOR theirs into it)


def _lib():
    from dust_amd import _lib as L

    lib = L.load()
    lib.dust_debug_philox.argtypes = [C.c_int, C.c_ulonglong, C.c_void_p, C.c_int, C.c_void_p]
    lib.dust_debug_philox.restype = C.c_int
    return lib


def dev_call(kind, key, ctr):
    """dust_debug_philox: kind 0 / 1 -> uint32 words [n][4] (7 / 10 rounds), 2 -> normal4 [n][4], 3 -> normal8 [n][8] (fp32)."""
    ctr = np.ascontiguousarray(ctr, np.uint32).reshape(-1, 4)
    out = np.zeros((len(ctr), 8 if kind == 3 else 4), np.uint32 if kind < 2 else np.float32)
    assert _lib().dust_debug_philox(kind, int(key) & 0xFFFFFFFFFFFFFFFF, ctr.ctypes.data, len(ctr), out.ctypes.data) == 0
    return out


def dev_normals(kind, key, ctr):
    """A normals source for philox_ref.assemble: the device's own fp32 normals."""
    return dev_call(3 if kind == pr.NORMAL8 else 2, key, ctr)


# ---- a. the generator
def test_device_generator_equals_host_replica():
    """Words bit for bit at 7 and 10 rounds (random counters, the edge words 0 and 0xffffffff, keys with the high word set); normals
    within 1e-5 max(1, |z|) of the float64 Box-Muller of the same uniforms - which pins radius / angle halves and the sin / cos order."""
    rng = np.random.default_rng(7)
    ctr = rng.integers(0, 2 ** 32, (4096, 4), dtype=np.uint64).astype(np.uint32)
    ctr[:16] = np.array([[0, 0, 0, 0], [0xFFFFFFFF] * 4, [0xFFFFFFFF, 0, 0xFFFFFFFF, 0], [0, 0xFFFFFFFF, 0, 0xFFFFFFFF]] * 4, np.uint32)
    for key in (0, 0xFFFFFFFFFFFFFFFF, SEED ^ pr.KEY_CTRP, SEED ^ pr.KEY_CTRD, SEED):
        assert np.array_equal(dev_call(0, key, ctr), pr.philox4x32(ctr, key, 7)), hex(key)
        assert np.array_equal(dev_call(1, key, ctr), pr.philox4x32_10(ctr, key)), hex(key)
        for kind, code in ((pr.NORMAL4, 2), (pr.NORMAL8, 3)):
            d, h = dev_call(code, key, ctr).astype(np.float64), pr.host_normals(kind, key, ctr)
            err = np.abs(d - h) / np.maximum(1.0, np.abs(h))
            assert err.max() < 1e-5, (hex(key), kind, err.max())


# ---- the scenes
FREE_STATE = np.array([-9.0, -9.0, 0.3, -0.2], np.float32)
OBST_STATE = np.array([-6.0, -4.6, 0.0, -0.3], np.float32)  # 0.3 above the obstacle at (-6, -6), drifting into it: crash or not is up to the draws


def _scene(S, N, M, H, scene, std, max_accel=10.0, seed=SEED, **extra):
    from oracle import grid_4x4_map

    obst = scene != "free"
    state = FREE_STATE if scene == "free" else OBST_STATE
    # (a target next to the start: the costs are the noise-driven deviations, not a terminal distance that no draw moves)
    target = (float(state[0]) + 0.5, float(state[1]) + 0.3, 0.0, 0.0)
    ctx = dict(model="particle", N=N, S=S, M=M, H=H, uncertain_params=("mass",), sampling=True, with_obstacle=obst, can_crash=scene == "crash",
               deterministic=False, noise_std=std, sigma_a=1.0, mass=2.0, dt=0.05, max_accel=max_accel, seed=seed, target=target)
    ctx.update(extra)
    ora = dict(model="particle", N=N, S=S, M=M, H=H, uncertain_params=("mass",), with_obstacle=obst, can_crash=scene == "crash", mass=2.0,
               dt=0.05, max_accel=max_accel, noise_std=std, grid=grid_4x4_map(), target=target)
    ora.update({k: v for k, v in extra.items() if k in ("control_type", "target", "w_state", "w_term")})
    rng = np.random.default_rng(S * 1000 + M * 10 + H)
    da = 2
    theta = (0.6 * rng.standard_normal((N, H, da))).astype(np.float32)
    params = (2.0 + 0.1 * rng.standard_normal((M, 1))).astype(np.float32)
    if extra.get("control_type") == "velocity":
        state = state[:2].copy()
    return ctx, ora, theta, params, state, (grid_4x4_map() if obst else None)


def _context(ctx, grid, theta):
    from dust_amd import Context

    c = Context(grid=grid, **ctx)
    c.set_theta(theta)
    c.set_a_mat(theta)
    return c


def _policy_actions(c, theta, tick, it):
    """The actions of a device-noise sample at stream position (tick, it), from the replica's policy layout and the device's normals."""
    z = pr.assemble(pr.policy_layout(c.cfg.seed, tick, it, c.S, c.N, c.H, 2), dev_normals)
    off = float(c.cfg.chol_a_off) if c.cfg.full_cov else None
    return pr.policy_actions(theta, z, [c.cfg.chol_a[0], c.cfg.chol_a[1]], off)


def _ctrl_z(form, S, N, M, H, tick=0, it=0, seed=SEED, G=None):
    lay = pr.ctrl_pair_path(seed, tick, it, S, N, M, H, G) if G is not None else pr.ctrl_layout(form, seed, tick, it, S, N, M, H)
    return pr.assemble(lay, dev_normals).astype(np.float32)


# ---- b. the policy layout
@pytest.mark.parametrize("a_cov", [None, ((1.0, 0.6), (0.6, 2.0))])
def test_policy_noise_layout(a_cov):
    """likelihood_sample(want_actions=True) with device noise: actions == theta + L z_replica(device normals) bit for bit, diagonal and full
    2 x 2 covariance (rollout.hpp's Philox staging: block j >> 3, counter (j8, s N + n, iter, tick), an odd column's partner draw)."""
    S, N, M, H = 64, 5, 2, 13
    ctx, _, theta, params, state, grid = _scene(S, N, M, H, "free", (0.6, 0.4), **({} if a_cov is None else dict(a_cov=np.array(a_cov, np.float32))))
    c = _context(ctx, grid, theta)
    assert bool(c.cfg.full_cov) == (a_cov is not None)
    for it in range(2):
        _, act = c.likelihood_sample(state, None, params, want_actions=True)
        assert np.array_equal(act, _policy_actions(c, theta, 0, it)), it
    c.close()


# ---- c. lean kernel, inline draws (+ h. sensitivity)
# (name, S, N, M, H, scene, noise_std, max_accel): G from rollout_args (tests/test_philox_ref_cpu.py pins it)
LEAN_CASES = [
    # G = 1, one pair (0, 1): pair path only; S N = 240
    ("M2_free", 48, 5, 2, 24, "free", (0.6, 0.4), 10.0),
    # G = 1, pair (0, 1) + sample 2 in the one-sample loop, odd H (the pair's last block serves one step)
    ("M3_obst_H23", 40, 6, 3, 23, "obst", (0.6, 0.4), 10.0),
    # G = 2: pairs (0, 2), (1, 3); crashes
    ("M4_crash_G2", 64, 3, 4, 20, "crash", (0.0, 0.5), 10.0),
    # G = 2: pairs (0, 2), (1, 3) and samples 4, 5 one-sample in one launch; max_accel binding (noise before the u / m clamp)
    ("M6_G2_clamp", 64, 3, 6, 22, "crash", (0.6, 0.4), 0.3),
    # G = 1, one-sample loop only; S N = 600
    ("M1_S200", 200, 3, 1, 21, "obst", (0.0, 0.5), 10.0),
    # cfg3's M = 64, S = 64, H = 40 at N = 2: G = 4
    ("cfg3_G4", 64, 2, 64, 40, "crash", (0.6, 0.4), 10.0),
]


@pytest.mark.parametrize("policy", ["eps0", "device"])
@pytest.mark.parametrize("name,S,N,M,H,scene,std,max_accel", LEAN_CASES, ids=[c[0] for c in LEAN_CASES])
def test_lean_kernel_inline_control_noise(name, S, N, M, H, scene, std, max_accel, policy):
    """likelihood_sample, costs only: rollout.hpp's lean kernel draws the control noise inside its loops (the packed pair path for the
    pairs (m, m + G), the one-sample loop for what they leave over; eps0: rollout_stream_kernel, device policy noise: rollout_kernel).
    Costs equal the oracle fed the replica's Z, and a twin context fed Z through set_ctrl_noise (particle_general.hpp's recorded-draw
    branch); Z with the channels swapped, shifted by one step, or (G = 2) the pair partner keyed m + 1 must miss by > 100 TOL."""
    from oracle import Oracle

    ctx, ora, theta, params, state, grid = _scene(S, N, M, H, scene, std, max_accel)
    G = pr.lean_lane_groups("particle", S, M)
    c = _context(ctx, grid, theta)
    eps = np.zeros((S, N, H, 2), np.float32) if policy == "eps0" else None
    costs = c.likelihood_sample(state, eps, params)
    actions = np.broadcast_to(theta, (S, N, H, 2)).copy() if policy == "eps0" else _policy_actions(c, theta, 0, 0)
    z = _ctrl_z("lean", S, N, M, H)
    o = Oracle(**ora)
    ref = o.rollout_cost(state, actions, params, ctrl_noise=z)
    assert np.isfinite(costs).all()
    assert elemerr(costs, ref) < TOL, (name, policy, elemerr(costs, ref))
    if scene == "crash":
        assert ref.max() > 1e6, "the scene must have rollouts that crash"
    twin = _context(ctx, grid, theta)
    twin.set_ctrl_noise(z[None])
    assert elemerr(twin.likelihood_sample(state, eps, params), costs) < TOL
    twin.close()
    c.close()
    # h. the comparison can fail: each fault of the layout misses by far more than the tolerance
    bad = {"channels swapped": z[..., ::-1], "shifted one step": np.roll(z, 1, axis=0)}
    if G == 2:
        bad["partner keyed m + 1"] = _ctrl_z(None, S, N, M, H, G=1)
    for what, zb in bad.items():
        e = elemerr(costs, o.rollout_cost(state, actions, params, ctrl_noise=np.ascontiguousarray(zb)))
        assert e > 100 * TOL, (name, what, e)


# ---- d. full kernel
@pytest.mark.parametrize("ctrl_penalty", [1.0, 0.5])
def test_full_kernel_inline_control_noise(ctrl_penalty):
    """disco_forward with omega (and a control penalty: the a_reg term): rollout.hpp's full kernel, every rollout in the one-sample loop
    ("ctrd" normal4 blocks) - costs and omega against the oracle."""
    from oracle import Oracle

    S, N, M, H = 64, 3, 3, 23
    ctx, ora, theta, params, state, grid = _scene(S, N, M, H, "crash", (0.6, 0.4), ctrl_penalty=ctrl_penalty)
    c = _context(ctx, grid, theta)
    rng = np.random.default_rng(11)
    actions = (theta[None] + rng.standard_normal((S, N, H, 2))).astype(np.float32)
    costs, _, _, omega = c.disco_forward(state, actions, params)
    z = _ctrl_z("full", S, N, M, H)
    o = Oracle(**ora)
    temp = float(c.cfg.temperature)
    a_reg = float(np.float32(temp * (1.0 - ctrl_penalty)))
    ref = o.rollout_cost(state, actions, params, a_reg, theta, None, np.ones(2, np.float32), ctrl_noise=z)
    assert ref.min() < 1e6 < ref.max()
    assert elemerr(costs, ref) < TOL, elemerr(costs, ref)
    om, _, _ = o.disco_weights(ref, actions, np.zeros(H * 2, np.float32), temp, theta)
    assert relerr(omega, om) < 2e-4
    # (the lean kernel's layout is not this one: the pairs would draw other normals)
    assert elemerr(costs, o.rollout_cost(state, actions, params, a_reg, theta, None, np.ones(2, np.float32), ctrl_noise=_ctrl_z("lean", S, N, M, H))) > 100 * TOL
    c.close()


# ---- e. particle_general.hpp's Philox branch
@pytest.mark.parametrize("control", ["acceleration", "velocity"])
def test_general_kernel_philox_branch(control):
    """Stored states (disco_forward(want_states=True)) and velocity control run particle_general.hpp; its Philox branch draws one
    normal8 block per four steps: costs and states against the oracle at H = 23 (H % 4 = 3: the last block serves three steps)."""
    from oracle import Oracle

    S, N, M, H = 64, 3, 4, 23
    extra = {} if control == "acceleration" else dict(control_type="velocity", target=(4.0, 4.5), w_state=(0.5, 0.5), w_term=(1e3, 1e3))
    ctx, ora, theta, params, state, grid = _scene(S, N, M, H, "crash", (0.6, 0.4), **extra)
    c = _context(ctx, grid, theta)
    actions = np.broadcast_to(theta, (S, N, H, 2)).copy()
    costs, states, _, _ = c.disco_forward(state, actions, params, want_states=True)
    z = _ctrl_z("general", S, N, M, H)
    o = Oracle(**ora)
    ref, ref_states = o.rollout_cost(state, actions, params, want_states=True, ctrl_noise=z)
    assert elemerr(costs, ref) < TOL, elemerr(costs, ref)
    assert np.abs(states - ref_states).max() < 1e-5 * max(1.0, np.abs(ref_states).max())
    assert elemerr(costs, o.rollout_cost(state, actions, params, ctrl_noise=_ctrl_z("full", S, N, M, H))) > 100 * TOL
    c.close()


# ---- f. stream positions and the product tick
def test_stream_positions():
    """Three consecutive samples draw at (tick, iter) = (0, 0), (0, 1), (0, 2); after svmpc_forward the next one draws at (1, 0)."""
    from oracle import Oracle

    S, N, M, H = 64, 3, 2, 12
    ctx, ora, theta, params, state, grid = _scene(S, N, M, H, "obst", (0.6, 0.4))
    c = _context(ctx, grid, theta)
    c.set_prior(theta)
    o = Oracle(**ora)
    for tick, it in ((0, 0), (0, 1), (0, 2), (1, 0)):
        if (tick, it) == (1, 0):
            c.svmpc_forward()
        th = c.get_theta()
        costs = c.likelihood_sample(state, None, params)
        ref = o.rollout_cost(state, _policy_actions(c, th, tick, it), params, ctrl_noise=_ctrl_z("lean", S, N, M, H, tick, it))
        assert elemerr(costs, ref) < TOL, (tick, it)
    c.close()


@pytest.mark.parametrize("no_fuse", ["0", "1"])
def test_noisy_particle_tick_replayed_through_oracle(no_fuse, monkeypatch):
    """One noisy Particle svmpc_tick(state, K = 2) replayed through the oracle with the replica's policy and control draws (rollouts,
    score, K1 phi, SGD, forward), as test_philox_tick_replayed_through_oracle does for the policy noise alone; the first iteration's
    costs at TOL, the whole tick at 2e-3 with its argmax rule.  DUST_NO_FUSE=1: the unfused launch sequence."""
    from oracle import Oracle

    if no_fuse == "1":
        monkeypatch.setenv("DUST_NO_FUSE", "1")
    else:
        monkeypatch.delenv("DUST_NO_FUSE", raising=False)
    N, S, M, H, K = 32, 64, 2, 20, 2
    sig, lr, alpha = 5.0, 20.0, 1e-4
    ctx, ora, _, _, state, grid = _scene(S, N, M, H, "obst", (0.6, 0.4), kernel="K1", lr=lr, alpha=alpha, sigma_a=sig, sigma_p=sig)
    rng = np.random.default_rng(17)
    mu = rng.standard_normal((N, H, 2)).astype(np.float32)
    theta = (mu + 0.5 * rng.standard_normal((N, H, 2))).astype(np.float32)
    params = (2.0 + 0.1 * rng.standard_normal((K, M, 1))).astype(np.float32)
    prod = _context(ctx, grid, theta)
    prod.set_prior(mu)
    a_seq, pw = prod.svmpc_tick(state, K, None, params)
    th_prod = prod.get_theta()
    prod.close()
    first = _context(ctx, grid, theta)
    first.set_prior(mu)
    first.svmpc_optimize(state, 1, None, params[:1])
    costs_first = first.get_costs()
    cfg = first.cfg
    first.close()
    o = Oracle(**ora)
    sg = np.full(2, sig, np.float32)
    th, mix = theta.copy(), np.ones(N, np.float32)
    for k in range(K):
        z = pr.assemble(pr.policy_layout(cfg.seed, 0, k, S, N, H, 2), dev_normals)
        actions = pr.policy_actions(th, z, [cfg.chol_a[0], cfg.chol_a[1]])
        costs = o.rollout_cost(state, actions, params[k], ctrl_noise=_ctrl_z("lean", S, N, M, H, 0, k))
        if k == 0:
            assert elemerr(costs_first, costs) < TOL, elemerr(costs_first, costs)
        _, _, sc = o.score(th, mu, mix, sg, costs, actions, alpha, sg)
        th = o.sgd(th, o.phi_k1(th, sc), lr)
    r = o.forward(costs, th, mu, mix, sg, alpha)
    scale = np.abs(r["theta"]).max()
    assert np.abs(th_prod - r["theta"]).max() / scale < 2e-3
    srt = np.sort(r["p_weights"])
    if srt[-1] > 1.5 * srt[-2]:
        assert int(np.argmax(pw)) == r["i_star"]
        assert np.abs(a_seq - r["a_seq"]).max() / scale < 2e-3


# ---- g. sharding
def test_sharded_noisy_tick_equals_unsharded():
    """A world-2 DeviceShard / LocalComm noisy Particle tick with device noise equals the unsharded tick (the draws are keyed by the
    GLOBAL particle index n0 + local): a_seq bit for bit, p_weights at 1e-5."""
    from dust_amd import Context
    from dust_amd.parallel import DeviceShard, LocalComm, tick

    N, S, M, H, K = 64, 64, 4, 16, 2
    ctx, _, theta, _, state, grid = _scene(S, N, M, H, "obst", (0.6, 0.4), kernel="K1", lr=0.5, sigma_p=1.0)
    rng = np.random.default_rng(5)
    mu = rng.standard_normal((N, H, 2)).astype(np.float32)
    params = (2.0 + 0.1 * rng.standard_normal((K, M, 1))).astype(np.float32)
    ref = Context(grid=grid, **ctx)
    ref.set_theta(theta); ref.set_prior(mu); ref.set_a_mat(theta)
    want = ref.svmpc_tick(state, K, None, params)
    rt = ref.get_theta()
    ref.close()
    shards = tuple(DeviceShard(dict(ctx, grid=grid), r, 2) for r in range(2))
    for sh in shards:
        sh.set_state(theta, mu, theta)
    a_seq, pw = tick(shards, LocalComm(), state, K, None, params, want_outputs=True)
    assert np.array_equal(a_seq, want[0])
    assert relerr(pw, want[1]) < 1e-5
    for sh in shards:
        sh.sync()
        assert elemerr(sh.ctx.get_theta(), rt) < 2e-6, sh.rank
        sh.ctx.close()
