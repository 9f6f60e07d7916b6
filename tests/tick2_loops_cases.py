"""Cases of tests/test_gpu_tick2_loops.py, shared with tools/record_tick2_golden.py (which writes tests/golden/tick2_loops_<case>.npz
from the library it is pointed at): the smallest shapes at which the hot loops of dust_amd/csrc/tick2.hpp - the rollout waves' weighted
sums, the Stein pass, K x score - take each of their paths.  Every case is three svmpc_tick calls from a seeded start; the first runs the
plain kernels (the prior means do not alias the particles yet), the other two are tick2 launches.

Large arrays are kept as one CRC-32 per particle row (uint32 [N]): `costs` always, the [N, D] arrays at N >= 1000, and whatever else
has more than 16 384 elements."""
import os
import zlib

import numpy as np

from test_gpu_tick2 import _snapshot, _state

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

# name: (model, N, S, H, iters, caller-supplied noise, Context keywords)
CASES = {
    # N = 1024 is the only N whose steps hold no key past the last (steps * 64 == N): the UNMASKED Stein, prior and log-density
    # instances; four trips of four steps per Stein unit; three score generations
    "n1024_s64_h8_it3": ("pendulum", 1024, 64, 8, 3, False, {}),
    "n1024_s128_h30_it2": ("pendulum", 1024, 128, 30, 2, False, {}),  # the benchmark's row stride: D 30, Dp 31
    "n1000_s64_h8_it2": ("pendulum", 1000, 64, 8, 2, False, {}),  # masked keys inside the last trip of the Stein loop
    "n68_s64_h8_it2": ("pendulum", 68, 64, 8, 2, False, {}),  # almost every step past the last key: clamped rows, weight 0
    "n64_s40_h12_it2": ("pendulum", 64, 40, 12, 2, False, {}),  # 20 samples per lane: two groups of 8, a remainder of 4
    "n64_s96_h12_it2": ("pendulum", 64, 96, 12, 2, False, {}),  # a ragged second wave: 16 samples per lane there, no remainder
    "n64_s200_h12_it2": ("pendulum", 64, 200, 12, 2, False, {}),  # the s0 += 128 trip: full in the even wave, a bare remainder in the odd one
    "n64_s128_h15_it2_temp": ("pendulum", 64, 128, 15, 2, False, dict(temperature=0.5)),  # alpha * temp != 1: omega weights, a_mat
    "n64_s40_h15_it2_temp": ("pendulum", 64, 40, 15, 2, False, dict(temperature=0.5)),  # ... on a group that does not fill
    "particle_n64_s64_h16_it2": ("particle", 64, 64, 16, 2, False, {}),  # D 32, Dp 33: full rows
    "particle_n64_s64_h16_it2_imq": ("particle", 64, 64, 16, 2, False, dict(kernel="IMQ")),
    "n64_s128_h16_it2_eps": ("pendulum", 64, 128, 16, 2, True, {}),  # noise staged by all rollout waves in phase 4
    "n64_s45_h12_it2": ("pendulum", 64, 45, 12, 2, False, {}),  # odd S: 23 samples in the even lanes, 22 in the odd ones
}
KEYS = ("a_seq", "p_weights", "theta", "a_mat", "costs", "score", "phi", "ll", "lp")
PER_PARTICLE = ("theta", "a_mat", "score", "phi")  # [N, D]
CRC_ABOVE = 16384


def tick2_launches(name):
    return 2


def golden_path(name):
    return os.path.join(GOLDEN, "tick2_loops_%s.npz" % name)


def make(model, N, S, H, seed=0, **kw):
    """A seeded context (tests/test_gpu_tick2.py's _make, with every Context keyword open: `temperature`)"""
    from dust_amd import Context

    da = 1 if model == "pendulum" else 2
    rng = np.random.default_rng(seed)
    mu = rng.standard_normal((N, H, da)).astype(np.float32)
    th = (mu + 2 * rng.standard_normal((N, H, da))).astype(np.float32)
    if model == "particle":
        from oracle import grid_4x4_map

        kw = dict(kw, grid=grid_4x4_map())
    sig = 2.0 if model == "pendulum" else 5.0
    c = Context(model=model, N=N, S=S, M=1, H=H, lr=2.0 if model == "pendulum" else 100.0, sigma_a=sig, sigma_p=sig, seed=77, **kw)
    c.set_theta(th)
    c.set_prior(mu)
    c.set_a_mat(th)
    return c, rng


def _kept(key, v, N):
    v = np.ascontiguousarray(v)
    if key == "costs" or v.size > CRC_ABOVE or (N >= 1000 and key in PER_PARTICLE):
        rows = v.reshape(N, -1)
        return np.array([zlib.crc32(rows[n].tobytes()) for n in range(N)], np.uint32)
    return np.array(v, copy=True)


def run_case(name):
    """-> ({"t<i>_<key>": array or row CRCs}, tick_stats) of the case on the library that is loaded"""
    model, N, S, H, iters, ext, kw = CASES[name]
    c, rng = make(model, N, S, H, **kw)
    da = 1 if model == "pendulum" else 2
    st = _state(model)
    out = {}
    try:
        for t in range(3):
            eps = rng.standard_normal((iters, S, N, H, da)).astype(np.float32) if ext else None
            a_seq, pw = c.svmpc_tick(st, iters, eps=eps)
            snap = _snapshot(c)
            vals = dict(a_seq=a_seq, p_weights=pw, theta=snap["theta"], a_mat=snap["a_mat"], costs=snap["costs"], score=snap["score"],
                        phi=snap["phi"], ll=snap["ll"], lp=snap["lp"])
            for k in KEYS:
                assert np.isfinite(vals[k]).all(), (name, t, k)
                out["t%d_%s" % (t, k)] = _kept(k, vals[k], N)
        stats = c.tick_stats()
    finally:
        c.close()
    return out, stats
