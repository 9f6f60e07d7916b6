"""Host restatement of the device's Philox streams and of the noise layouts that draw from them (test infrastructure, not a test).

Written from the published algorithm (Salmon et al., "Parallel random numbers: as easy as 1, 2, 3", SC'11 - the Random123 Philox4x32
round with its Weyl key bump) and from the comments of dust_amd/csrc/common.hpp, rollout.hpp and particle_general.hpp, in numpy
uint32 / uint64 arithmetic.  It states independently WHICH Philox block (key, counter) and which lane of it serves every element of
every noise tensor the device draws; the GPU tests fetch the device's own normals at those counters (dust_debug_philox) and compare
the kernels with the CPU oracle fed the assembled draws.

Layouts (r = (m S + s) N + n the rollout index, n the GLOBAL particle index n0 + local; tick / iter the context's stream position):
  * policy noise [S][N][H*da]: element j of row (s, n) is lane j & 7 of philox_normal8(seed; j >> 3, s N + n, iter, tick); with a full
    2 x 2 action covariance an odd column also takes its partner draw j - 1 (the same block);
  * control noise, rollout.hpp packed pair path: the pair (m, m + G) of a lane draws ONE philox_normal8 block per two steps,
    key seed ^ "ctrp", counter (lo(rN), hi(rN) ^ (t / 2) << 8, iter, tick), rN the pair's FIRST rollout; step t + q, q = t & 1, takes
    lanes 4q (+2 for the partner) + channel;
  * control noise, rollout.hpp one-sample loop: one philox_normal4 block per two steps of rollout r, key seed ^ "ctrd", counter
    (lo(r), hi(r) ^ (t / 2) << 8, iter, tick), lane 2 (t & 1) + channel;
  * control noise, particle_general.hpp: one philox_normal8 block per four steps of rollout r, key seed ^ "ctrd", counter
    (lo(r), hi(r) ^ (t / 4) << 8, iter, tick), lane 2 (t & 3) + channel.
"""
import numpy as np

U32 = np.uint64(0xFFFFFFFF)
_M0, _M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)  # Philox4x32 multipliers
_W0, _W1 = np.uint64(0x9E3779B9), np.uint64(0xBB67AE85)  # Weyl key increments
KEY_CTRP = 0x63747270 << 32  # "ctrp": control noise of the packed pair path
KEY_CTRD = 0x63747264 << 32  # "ctrd": control noise of the one-sample loop and of particle_general.hpp
NORMAL4, NORMAL8 = 4, 8      # the two normal generators, named by their block size


def philox4x32(ctr, key, rounds):
    """Philox4x32-R: ctr [..., 4] counter words, key a 64-bit key (k0 = low word, k1 = high word) -> [..., 4] uint32 output words."""
    c = np.asarray(ctr, np.uint64) & U32
    key = np.uint64(int(key) & 0xFFFFFFFFFFFFFFFF)
    k0, k1 = key & U32, key >> np.uint64(32)
    c0, c1, c2, c3 = c[..., 0], c[..., 1], c[..., 2], c[..., 3]
    for _ in range(rounds):
        p0, p1 = _M0 * c0, _M1 * c2  # 32 x 32 -> 64 bits: no wrap in uint64
        hi0, lo0, hi1, lo1 = p0 >> np.uint64(32), p0 & U32, p1 >> np.uint64(32), p1 & U32
        c0, c1, c2, c3 = hi1 ^ c1 ^ k0, lo1, hi0 ^ c3 ^ k1, lo0
        k0, k1 = (k0 + _W0) & U32, (k1 + _W1) & U32
    return np.stack([c0, c1, c2, c3], -1).astype(np.uint32)


def philox4x32_10(ctr, key):
    return philox4x32(ctr, key, 10)


def _fp32_half_step(n, bits):
    """u = (n + 1/2) 2^-bits as the device forms it: fmaf(float(n), 2^-bits, 2^-(bits+1)) - ONE rounding of the exact value to fp32."""
    return ((2.0 * np.asarray(n, np.float64) + 1.0) * 2.0 ** -(bits + 1)).astype(np.float32)


def uniforms4(words):
    """philox_normal4's four uniforms: the top 24 bits of each word (fp32; the odd ones are the angles, in revolutions)."""
    return _fp32_half_step(np.asarray(words, np.uint32) >> np.uint32(8), 24)


def uniforms8(words):
    """philox_normal8's uniforms: per word (radius from the low 16 bits, angle from the high 16 bits) -> [..., 4, 2] fp32."""
    w = np.asarray(words, np.uint32)
    return np.stack([_fp32_half_step(w & np.uint32(0xFFFF), 16), _fp32_half_step(w >> np.uint32(16), 16)], -1)


def _box_muller(u, a):
    """sqrt(-2 ln u) (cos 2 pi a, sin 2 pi a) in float64 from the device's fp32 uniforms."""
    u, a = np.asarray(u, np.float64), np.asarray(a, np.float64)
    ra = np.sqrt(-2.0 * np.log(u))
    return ra * np.cos(2.0 * np.pi * a), ra * np.sin(2.0 * np.pi * a)


def normal4(ctr, key):
    """philox_normal4 in float64: [..., 4] = (r0 cos a1, r0 sin a1, r2 cos a3, r2 sin a3), 7 Philox rounds."""
    u = uniforms4(philox4x32(ctr, key, 7))
    z0, z1 = _box_muller(u[..., 0], u[..., 1])
    z2, z3 = _box_muller(u[..., 2], u[..., 3])
    return np.stack([z0, z1, z2, z3], -1)


def normal8(ctr, key):
    """philox_normal8 in float64: [..., 8], word i gives (cos, sin) of radius low half / angle high half at 2i, 2i + 1."""
    ua = uniforms8(philox4x32(ctr, key, 7))
    zc, zs = _box_muller(ua[..., 0], ua[..., 1])
    return np.stack([zc, zs], -1).reshape(zc.shape[:-1] + (8,))


def host_normals(kind, key, ctr):
    """A normals source (see assemble): the host float64 normals of blocks ctr [n][4] under one key."""
    return normal8(ctr, key) if kind == NORMAL8 else normal4(ctr, key)


class Layout:
    """Which block serves each element of a noise tensor: kind (NORMAL4 / NORMAL8), key (uint64), ctr [..., 4] (uint32), lane (int),
    each of the tensor's shape."""

    def __init__(self, kind, key, ctr, lane):
        self.kind, self.key, self.ctr, self.lane = kind, key, ctr, lane
        self.shape = lane.shape

    def ids(self):
        """One row per element: (kind, key, c0, c1, c2, c3, lane) as uint64 - two elements share a row iff they share a draw."""
        cols = [self.kind, self.key] + [self.ctr[..., i] for i in range(4)] + [self.lane]
        return np.stack([np.broadcast_to(np.asarray(c).astype(np.uint64), self.shape).reshape(-1) for c in cols], -1)

    def draw_ids(self):
        """The same without the generator kind: elements that read the same lane of the same Philox words (normal4 and normal8 of one
        key and counter are functions of the same four words)."""
        return self.ids()[:, 1:]


def _ctr(c0, c1, c2, c3, shape):
    out = np.empty(shape + (4,), np.uint32)
    for i, c in enumerate((c0, c1, c2, c3)):
        out[..., i] = np.broadcast_to(np.asarray(c, np.uint64) & U32, shape)
    return out


def policy_layout(seed, tick, it, S, N, H, da, n0=0, n_local=None):
    """Policy noise [S][n_local][H*da] of a sample at stream position (tick, it): block j >> 3 of row (s, n), lane j & 7."""
    nl = N - n0 if n_local is None else n_local
    D = H * da
    s = np.arange(S, dtype=np.uint64)[:, None, None]
    n = (n0 + np.arange(nl, dtype=np.uint64))[None, :, None]
    j = np.arange(D, dtype=np.uint64)[None, None, :]
    shape = (S, nl, D)
    ctr = _ctr(j >> np.uint64(3), s * np.uint64(N) + n, it, tick, shape)
    lane = np.broadcast_to((j & np.uint64(7)).astype(np.int64), shape)
    return Layout(np.full(shape, NORMAL8, np.int64), np.full(shape, int(seed) & 0xFFFFFFFFFFFFFFFF, np.uint64), ctr, lane)


def policy_actions(theta, z, chol_a, chol_off=None):
    """theta [n][H][da] + L z, z [S][n][H*da] normals in the policy layout, in the device's fp32 order: diagonal th + l_d z; a full 2 x 2
    L (chol_off = L[1][0]) gives the odd column th + (chol_off z[j - 1] + l_1 z[j]), its partner draw from the same block."""
    th = np.asarray(theta, np.float32)
    S = z.shape[0]
    nl, H, da = th.shape
    zz = np.asarray(z, np.float32).reshape(S, nl, H, da)
    l = np.asarray(chol_a, np.float32).reshape(-1)[:da]
    if chol_off is None or da != 2:
        return (th[None] + l * zz).astype(np.float32)
    out = np.empty((S, nl, H, da), np.float32)
    out[..., 0] = th[None, ..., 0] + l[0] * zz[..., 0]
    out[..., 1] = th[None, ..., 1] + (np.float32(chol_off) * zz[..., 0] + l[1] * zz[..., 1])
    return out


def lean_lane_groups(model, S, M, costs_in=False, sigma_weights=False):
    """The dynamics-sample lane groups G of a rollout launch (dust_amd.hip rollout_args): G doubles while 2G <= M and roundup64(S) 2G <= 256
    and, for Particle, 4G <= M (the packed pair path wants >= 2 samples per lane); none with injected costs or sigma-point weights."""
    if costs_in or sigma_weights:
        return 1
    sub = (S + 63) // 64 * 64
    G = 1
    while 2 * G <= M and sub * 2 * G <= 256 and (model != "particle" or 4 * G <= M):
        G *= 2
    return G


def pair_roles(M, G):
    """Per dynamics sample m of the packed pair path: (role, first) - role 0 / 1 for the first / partner rollout of a pair (m, m + G),
    -1 for the samples the pairs leave to the one-sample loop; first = the pair's first sample.  Group g walks m = g, g + 2G, ... while
    m + G < M (rollout.hpp)."""
    role, first = np.full(M, -1, np.int64), np.arange(M, dtype=np.int64)
    for g in range(G):
        m = g
        while m + G < M:
            role[m], role[m + G] = 0, 1
            first[m], first[m + G] = m, m
            m += 2 * G
    return role, first


def _rollout_grid(S, N, M, H, n0, n_local):
    nl = N - n0 if n_local is None else n_local
    m = np.arange(M, dtype=np.int64)[None, :, None, None, None]
    s = np.arange(S, dtype=np.int64)[None, None, :, None, None]
    n = (n0 + np.arange(nl, dtype=np.int64))[None, None, None, :, None]
    t = np.arange(H, dtype=np.int64)[:, None, None, None, None]
    ch = np.arange(2, dtype=np.int64)[None, None, None, None, :]
    return (H, M, S, nl, 2), m, s, n, t, ch


def _ctrl_counter(r, step_block, tick, it, shape):
    r = np.asarray(r, np.uint64)
    c1 = (r >> np.uint64(32)) ^ ((np.asarray(step_block, np.uint64) << np.uint64(8)) & U32)
    return _ctr(r & U32, c1, it, tick, shape)


def _flat(layout, shape):
    """[H][M][S][nl][2] -> [H][M*S*nl][2] (rollout rows in the oracle's r = (m S + s) N + n order)."""
    H, M, S, nl, _ = shape
    f = lambda x: np.broadcast_to(x, shape).reshape(H, M * S * nl, 2)
    return Layout(f(layout.kind), f(layout.key), np.broadcast_to(layout.ctr, shape + (4,)).reshape(H, M * S * nl, 2, 4), f(layout.lane))


def ctrl_one_sample(seed, tick, it, S, N, M, H, n0=0, n_local=None):
    """Control noise [H][M*S*n_local][2] of rollout.hpp's one-sample loop (every rollout of the full kernel)."""
    shape, m, s, n, t, ch = _rollout_grid(S, N, M, H, n0, n_local)
    r = m * S * N + s * N + n
    ctr = _ctrl_counter(r, t >> 1, tick, it, shape)
    key = np.full(shape, (int(seed) ^ KEY_CTRD) & 0xFFFFFFFFFFFFFFFF, np.uint64)
    return _flat(Layout(np.full(shape, NORMAL4, np.int64), key, ctr, np.broadcast_to(2 * (t & 1) + ch, shape)), shape)


def ctrl_pair_path(seed, tick, it, S, N, M, H, G, n0=0, n_local=None):
    """Control noise [H][M*S*n_local][2] of the lean kernel: the packed pairs (m, m + G) draw "ctrp" blocks keyed by the pair's first
    rollout, the samples the pairs leave over draw the one-sample loop's "ctrd" blocks."""
    shape, m, s, n, t, ch = _rollout_grid(S, N, M, H, n0, n_local)
    role, first = pair_roles(M, G)
    role_m, first_m = role[m], first[m]
    paired = role_m >= 0
    r = m * S * N + s * N + n
    rN = first_m * S * N + s * N + n
    ctr = np.where(paired[..., None], _ctrl_counter(rN, t >> 1, tick, it, shape), _ctrl_counter(r, t >> 1, tick, it, shape))
    key = np.where(paired, np.uint64((int(seed) ^ KEY_CTRP) & 0xFFFFFFFFFFFFFFFF), np.uint64((int(seed) ^ KEY_CTRD) & 0xFFFFFFFFFFFFFFFF))
    lane = np.where(paired, 4 * (t & 1) + 2 * np.maximum(role_m, 0) + ch, 2 * (t & 1) + ch)
    kind = np.where(paired, NORMAL8, NORMAL4)
    return _flat(Layout(np.broadcast_to(kind, shape), np.broadcast_to(key, shape), ctr, np.broadcast_to(lane, shape)), shape)


def ctrl_general(seed, tick, it, S, N, M, H, n0=0, n_local=None):
    """Control noise [H][M*S*n_local][2] of particle_general.hpp's Philox branch (stored states, velocity control)."""
    shape, m, s, n, t, ch = _rollout_grid(S, N, M, H, n0, n_local)
    r = m * S * N + s * N + n
    ctr = _ctrl_counter(r, t >> 2, tick, it, shape)
    key = np.full(shape, (int(seed) ^ KEY_CTRD) & 0xFFFFFFFFFFFFFFFF, np.uint64)
    return _flat(Layout(np.full(shape, NORMAL8, np.int64), key, ctr, np.broadcast_to(2 * (t & 3) + ch, shape)), shape)


def ctrl_layout(form, seed, tick, it, S, N, M, H, model="particle", n0=0, n_local=None):
    """The control-noise layout of a launch: form "lean" (inline draws, lean kernel: pairs + leftovers, G by lean_lane_groups),
    "full" (inline draws, full kernel: one-sample loop only) or "general" (particle_general.hpp)."""
    if form == "lean":
        return ctrl_pair_path(seed, tick, it, S, N, M, H, lean_lane_groups(model, S, M), n0, n_local)
    if form == "full":
        return ctrl_one_sample(seed, tick, it, S, N, M, H, n0, n_local)
    if form == "general":
        return ctrl_general(seed, tick, it, S, N, M, H, n0, n_local)
    raise ValueError(form)


def assemble(layout, normals):
    """The noise tensor of a layout from a normals source normals(kind, key, ctr [n][4]) -> [n][kind] (the device hook or host_normals):
    every distinct block is evaluated once.  float64 (cast as the consumer needs; the device's normals are fp32 values)."""
    out = np.empty(layout.shape, np.float64)
    kind = np.broadcast_to(layout.kind, layout.shape)
    key = np.broadcast_to(layout.key, layout.shape)
    for k in np.unique(kind):
        for kv in np.unique(key[kind == k]):
            sel = (kind == k) & (key == kv)
            c = layout.ctr[sel]
            packed = np.stack([c[:, 0].astype(np.uint64) | (c[:, 1].astype(np.uint64) << np.uint64(32)),
                               c[:, 2].astype(np.uint64) | (c[:, 3].astype(np.uint64) << np.uint64(32))], -1)
            uniq, inv = np.unique(packed, axis=0, return_inverse=True)
            blocks = np.stack([uniq[:, 0] & U32, uniq[:, 0] >> np.uint64(32), uniq[:, 1] & U32, uniq[:, 1] >> np.uint64(32)], -1).astype(np.uint32)
            z = np.asarray(normals(int(k), int(kv), blocks), np.float64).reshape(len(blocks), int(k))
            out[sel] = z[inv.reshape(-1), np.asarray(layout.lane)[sel]]
    return out
