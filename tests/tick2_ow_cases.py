"""Cases of tests/test_gpu_tick2_owner_waves.py, shared with tools/record_tick2_golden.py (which writes tests/golden/tick2_ow_<case>.npz
from the library it is pointed at).  Every case is three calls' worth of ticks from a seeded start; the first tick runs the plain
kernels (the prior means do not alias the particles yet), the rest run dust_amd/csrc/tick2.hpp."""
import os

import numpy as np

from test_gpu_tick2 import _make, _snapshot, _state

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

# name: (model, N, S, H, iters, M, caller-supplied noise, Context keywords, script)
#   script "ticks": three svmpc_tick calls (two tick2 launches);
#          "opt_fwd": svmpc_tick(1 iteration), svmpc_optimize(iters) + svmpc_forward(), svmpc_optimize(iters) (three tick2 launches)
CASES = {
    "n64_s128_h15_it3": ("pendulum", 64, 128, 15, 3, 1, False, {}, "ticks"),
    "n96_s64_h20_it3_adam": ("pendulum", 96, 64, 20, 3, 1, False, dict(optimizer="Adam"), "ticks"),
    "n64_s96_h12_m4_it2": ("pendulum", 64, 96, 12, 2, 4, False, {}, "ticks"),
    "n64_s128_h16_it1_eps": ("pendulum", 64, 128, 16, 1, 1, True, {}, "ticks"),
    "n64_s128_h16_it2_eps": ("pendulum", 64, 128, 16, 2, 1, True, {}, "ticks"),
    "n128_s128_h30_it2_imq_wprior": ("pendulum", 128, 128, 30, 2, 1, False, dict(kernel="IMQ", weighted_prior=True), "ticks"),
    "particle_n64_s64_h12_it2_rollmean": ("particle", 64, 64, 12, 2, 1, False, dict(roll="mean"), "ticks"),
    "n64_h15_adam_opt2_fwd": ("pendulum", 64, 128, 15, 2, 1, False, dict(optimizer="Adam"), "opt_fwd"),
}
KEYS = ("a_seq", "p_weights", "theta", "a_mat", "costs", "score", "phi", "ll", "lp")


def tick2_launches(name):
    return 3 if CASES[name][8] == "opt_fwd" else 2


def golden_path(name):
    return os.path.join(GOLDEN, "tick2_ow_%s.npz" % name)


def run_case(name):
    """-> ({"t<i>_<key>": array}, tick_stats) of the case on the library that is loaded"""
    model, N, S, H, iters, M, ext, kw, script = CASES[name]
    c, rng = _make(model, N, S, H, M=M, **kw)
    da = 1 if model == "pendulum" else 2
    st = _state(model)

    def inputs(n_it):
        eps = rng.standard_normal((n_it, S, N, H, da)).astype(np.float32) if ext else None
        params = None
        if M > 1:
            params = (1.0 + 0.1 * rng.standard_normal((n_it, M, 1 if model == "particle" else 2))).astype(np.float32)
        return eps, params

    out = {}

    def record(t, a_seq, pw):
        snap = _snapshot(c)
        vals = dict(a_seq=a_seq, p_weights=pw, theta=snap["theta"], a_mat=snap["a_mat"], costs=snap["costs"], score=snap["score"],
                    phi=snap["phi"], ll=snap["ll"], lp=snap["lp"])
        for k in KEYS:
            if vals[k] is not None:
                out["t%d_%s" % (t, k)] = np.array(vals[k], copy=True)

    try:
        if script == "ticks":
            for t in range(3):
                eps, params = inputs(iters)
                a_seq, pw = c.svmpc_tick(st, iters, eps=eps, params=params)
                record(t, a_seq, pw)
        else:
            eps, params = inputs(1)
            a_seq, pw = c.svmpc_tick(st, 1, eps=eps, params=params)
            record(0, a_seq, pw)
            eps, params = inputs(iters)
            c.svmpc_optimize(st, iters, eps=eps, params=params)
            a_seq, pw = c.svmpc_forward()  # (no getter in between: the forward stays a one-launch tick without iterations)
            record(1, a_seq, pw)
            eps, params = inputs(iters)
            c.svmpc_optimize(st, iters, eps=eps, params=params)
            record(2, None, None)  # behind the optimize-only exit: particles and moments as the iterations left them
        stats = c.tick_stats()
    finally:
        c.close()
    return out, stats
