"""The host restatement of the device's Philox streams and noise layouts (tests/philox_ref.py), on the CPU: the generator against
known-answer words, the layouts' injectivity within a launch and across stream positions, and the lane-group rule G that makes the
pair partner part of the control-noise layout."""
import numpy as np
import pytest

import philox_ref as pr

# Philox4x32-10 known answers: ((c0, c1, c2, c3), key = k1 << 32 | k0, (out0..out3)), computed with rocRAND's host-callable
# rocrand_philox4x32_10.h (philox4x32_10_engine::ten_rounds); the first three are also Random123's published kat_vectors.
PHILOX10_KAT = [
    ((0x00000000, 0x00000000, 0x00000000, 0x00000000), 0x0000000000000000, (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff, 0xffffffff, 0xffffffff, 0xffffffff), 0xffffffffffffffff, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), 0x299f31d0a4093822, (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
    ((0x00000007, 0x00000300, 0x00000002, 0x00000001), 0x637472700000002a, (0x2a19525a, 0x5651d4a8, 0xb99d4b6d, 0xd0e2fa91)),
    ((0x12345678, 0x9abcdef0, 0x00000000, 0xffffffff), 0x6374726400001092, (0x99566b1d, 0x50604180, 0xe6f3d7d8, 0xb276fbcb)),
]


@pytest.mark.parametrize("ctr,key,want", PHILOX10_KAT)
def test_philox4x32_10_known_answers(ctr, key, want):
    assert tuple(int(w) for w in pr.philox4x32_10(np.array(ctr, np.uint32), key)) == want
    # batched: the same words in any position of a block array
    got = pr.philox4x32(np.array([ctr, ctr], np.uint32), key, 10)
    assert got.dtype == np.uint32 and np.array_equal(got[0], got[1]) and tuple(int(w) for w in got[1]) == want


def test_uniforms_and_normals_as_the_device_forms_them():
    """24-bit uniforms for normal4 (rounded once to fp32, as fmaf rounds them), 16-bit radius (low half) and angle (high half) for
    normal8; the float64 normals are Box-Muller pairs of them with the law of standard normals."""
    w = np.array([0x00000000, 0xFFFFFFFF, 0x0000FFFF, 0xFFFF0000], np.uint32)
    u4 = pr.uniforms4(w)
    assert u4.dtype == np.float32 and np.all(u4 > 0) and np.all(u4 <= 1)
    # the top word 2^24 - 1 gives 1 - 2^-25, halfway between 1 - 2^-24 and 1: fmaf rounds the tie to even, u = 1 (radius 0)
    assert u4[0] == np.float32(2.0 ** -25) and u4[1] == np.float32(1.0) and u4[2] == np.float32(511 * 2.0 ** -25)
    u8 = pr.uniforms8(w)
    assert u8.shape == (4, 2) and u8[2, 0] == np.float32(1 - 2.0 ** -17) and u8[2, 1] == np.float32(2.0 ** -17)
    assert u8[3, 0] == np.float32(2.0 ** -17) and u8[3, 1] == np.float32(1 - 2.0 ** -17)
    rng = np.random.default_rng(1)
    ctr = rng.integers(0, 2 ** 32, (20000, 4), dtype=np.uint64).astype(np.uint32)
    for kind in (pr.NORMAL4, pr.NORMAL8):
        z = pr.host_normals(kind, 0x6374727000000007, ctr)
        assert z.shape == (20000, kind)
        n = z.size
        assert abs(z.mean()) < 5 / np.sqrt(n) and abs(z.var() - 1) < 5 * np.sqrt(2 / n)
        # the two members of a Box-Muller pair and neighbouring pairs are uncorrelated
        assert abs(np.corrcoef(z[:, 0], z[:, 1])[0, 1]) < 5 / np.sqrt(len(z))
        assert abs(np.corrcoef(z[:, 0], z[:, 2])[0, 1]) < 5 / np.sqrt(len(z))
    # normal8: word i -> (r cos a, r sin a) at lanes 2i, 2i + 1
    u = pr.uniforms8(pr.philox4x32(ctr[:3], 5, 7))
    z = pr.normal8(ctr[:3], 5)
    ra = np.sqrt(-2 * np.log(u[..., 0].astype(np.float64)))
    assert np.allclose(z[:, 0::2], ra * np.cos(2 * np.pi * u[..., 1].astype(np.float64)), rtol=0, atol=1e-14)
    assert np.allclose(z[:, 1::2], ra * np.sin(2 * np.pi * u[..., 1].astype(np.float64)), rtol=0, atol=1e-14)


# (S, N, M, H): H odd / even / H % 4 != 0, M in {1, 2, 3, 4, 6, 8, 64}, S * N not a multiple of 64
LAYOUT_SHAPES = [(64, 5, 1, 23), (200, 3, 1, 6), (64, 3, 2, 24), (64, 3, 3, 23), (64, 4, 4, 22), (64, 3, 6, 21), (32, 3, 8, 10),
                 (8, 5, 8, 9), (64, 2, 64, 40), (16, 3, 64, 7)]


def _launch_ids(form, seed, tick, it, S, N, M, H, G=None):
    da = 2
    pol = pr.policy_layout(seed, tick, it, S, N, H, da).draw_ids()
    if G is not None:
        ctl = pr.ctrl_pair_path(seed, tick, it, S, N, M, H, G)
    else:
        ctl = pr.ctrl_layout(form, seed, tick, it, S, N, M, H)
    return np.concatenate([pol, ctl.draw_ids()])


def _distinct(ids):
    rows = np.ascontiguousarray(ids).view(np.dtype((np.void, ids.dtype.itemsize * ids.shape[1]))).reshape(-1)
    return len(np.unique(rows)) == len(rows)


@pytest.mark.parametrize("form,S,N,M,H", [(f,) + sh for f in ("lean", "full", "general") for sh in LAYOUT_SHAPES] +
                         [(f,) + sh for f in ("G2", "G4") for sh in LAYOUT_SHAPES if sh[2] >= 2 * int(f[1])])
def test_layouts_are_injective_within_and_across_launches(form, S, N, M, H):
    """No two (rollout, step, channel) elements - nor a policy-noise element - of one launch read the same (key, counter, lane), and
    no element of launch (tick, iter) shares one with (tick, iter + 1) or (tick + 1, 0); "G2" / "G4": the pair path with that many lane
    groups whatever the shape's own G."""
    G = int(form[1]) if form in ("G2", "G4") else None
    seed = 0x0123456789ABCDEF
    a = _launch_ids(form, seed, 3, 5, S, N, M, H, G)
    assert len(a) == S * N * H * 2 + M * S * N * H * 2
    assert _distinct(a), (form, S, N, M, H)
    for tick, it in ((3, 6), (4, 0)):
        b = _launch_ids(form, seed, tick, it, S, N, M, H, G)
        assert _distinct(np.concatenate([a, b])), (form, tick, it)


def test_pair_layout_shapes():
    """The pair path's block rule on a small case, element by element: pair (0, 2) and (1, 3) at G = 2, M = 6 leaves 4 and 5 to the
    one-sample loop; the partner reads lanes 2, 3 / 6, 7 of its first rollout's block."""
    S, N, M, H, G, seed = 2, 3, 6, 3, 2, 9
    role, first = pr.pair_roles(M, G)
    assert role.tolist() == [0, 0, 1, 1, -1, -1] and first.tolist() == [0, 1, 0, 1, 4, 5]
    lay = pr.ctrl_pair_path(seed, 1, 2, S, N, M, H, G)
    SN = S * N
    r = lambda m, s, n: m * SN + s * N + n
    # partner (m = 2) of pair (0, 2), step 1, channel 1: block of rollout r(0, s, n), step block 0, lane 4 + 2 + 1
    e = (1, r(2, 1, 2), 1)
    assert int(lay.key[e]) == seed ^ pr.KEY_CTRP and lay.ctr[e].tolist() == [r(0, 1, 2), 0, 2, 1] and int(lay.lane[e]) == 7
    # leftover m = 5, step 2: one-sample block of its own rollout, step block 1 in the high counter word's bits 8..
    e = (2, r(5, 0, 1), 0)
    assert int(lay.key[e]) == seed ^ pr.KEY_CTRD and lay.ctr[e].tolist() == [r(5, 0, 1), 1 << 8, 2, 1] and int(lay.lane[e]) == 0
    assert int(lay.kind[e]) == pr.NORMAL4 and int(lay.kind[1, r(2, 1, 2), 1]) == pr.NORMAL8
    gen = pr.ctrl_general(seed, 1, 2, S, N, M, H + 4)
    e = (5, r(3, 1, 0), 1)  # step 5: block t / 4 = 1, lane 2 (t & 3) + 1
    assert gen.ctr[e].tolist() == [r(3, 1, 0), 1 << 8, 2, 1] and int(gen.lane[e]) == 3
    # the global particle index: a shard's rows are the same elements of the unsharded layout
    full = pr.ctrl_pair_path(seed, 1, 2, S, N, M, H, G)
    part = pr.ctrl_pair_path(seed, 1, 2, S, N, M, H, G, n0=1, n_local=2)
    sel = np.array([r(m, s, n) for m in range(M) for s in range(S) for n in (1, 2)])
    assert np.array_equal(part.ctr, full.ctr[:, sel]) and np.array_equal(part.lane, full.lane[:, sel])
    pol = pr.policy_layout(seed, 1, 2, S, N, H, 2, n0=1, n_local=2)
    assert np.array_equal(pol.ctr, pr.policy_layout(seed, 1, 2, S, N, H, 2).ctr[:, 1:3])


@pytest.mark.parametrize("S,M,G", [(64, 2, 1), (64, 3, 1), (64, 4, 2), (64, 6, 2), (200, 1, 1), (64, 64, 4), (64, 8, 4), (128, 8, 2),
                                   (32, 16, 4), (64, 16, 4)])
def test_lane_group_rule_on_the_gpu_test_shapes(S, M, G):
    """rollout_args' G for the Particle shapes of tests/test_gpu_ctrl_noise.py: it decides which rollout a pair partner's draws are keyed
    by, so it is part of the layout."""
    assert pr.lean_lane_groups("particle", S, M) == G
    assert pr.lean_lane_groups("particle", S, M, costs_in=True) == 1
    if M >= 2 and S <= 64:
        assert pr.lean_lane_groups("pendulum", S, M) >= G  # (Pendulum has no pair-path floor: more groups where M allows)
