"""The batched SVMPC tick against the same work done serially, closed loop: every period hands the plant states in and reads the chosen
action sequences back.  Pendulum, device-drawn noise, one SVGD step per tick, at
  demo  - demo/pendulum_config.yaml's shape: N 3, S 128, M 8 (length, mass sampled: [M, 2] rows per tick from the host), H 30;
  cfg1  - BASELINE config 1's shape: N 32, S 128, M 1, H 15;
B in {1, 4, 16, 64, 256}:
  (a) ONE dust_svmpc_batch_tick of B environments per period;
  (b) B lone dust_svmpc_tick calls per period, B contexts ticked in turn (each on its own stream).
Both legs run in the same process, alternating, REPS times each after a warm-up of every shape; a leg's time is a host clock around
`ticks` periods (every call waits for its outputs).  Printed: the median environment-ticks/s of each leg, the spread (min .. max over
the repeats) and the ratio of the medians.
    python tools/svmpc_batch_time.py [seconds per window, default 1.0] [largest B, default 256]"""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from dust_amd import Context

WINDOW = float(sys.argv[1]) if len(sys.argv) > 1 else 1.0
BMAX = int(sys.argv[2]) if len(sys.argv) > 2 else 256
REPS = 3
SHAPES = {"demo": dict(N=3, S=128, M=8, H=30, uncertain_params=("length", "mass")), "cfg1": dict(N=32, S=128, M=1, H=15)}


def leg(fn, ticks):
    t0 = time.perf_counter()
    for _ in range(ticks):
        fn()
    return (time.perf_counter() - t0) / ticks


def ticks_for(fn):
    """periods per timed window: warm the shape up, then size the window from a short probe"""
    for _ in range(10):
        fn()
    return max(10, int(WINDOW / leg(fn, 10)) + 1)


print("shape B batch_env_ticks_per_s [min max] lone_env_ticks_per_s [min max] batch_us_per_period lone_us_per_period ratio", flush=True)
for name, shape in SHAPES.items():
    for B in (1, 4, 16, 64, 256):
        if B > BMAX:
            continue
        N, S, M, H = shape["N"], shape["S"], shape["M"], shape["H"]
        rng = np.random.default_rng(S + B)
        mu = rng.standard_normal((N, H, 1)).astype(np.float32)
        th = (mu + 2 * rng.standard_normal((N, H, 1))).astype(np.float32)
        states = (np.array([3.0, 0.0], np.float32) + 0.1 * rng.standard_normal((B, 2))).astype(np.float32)
        params = (1.0 + 0.1 * rng.standard_normal((B, 1, M, 2))).astype(np.float32) if M > 1 else None
        kw = dict(model="pendulum", kernel="K1", lr=2.0, sigma_a=2.0, sigma_p=2.0, **shape)
        lone = [Context(seed=3 + b, **kw) for b in range(B)]
        for c in lone:
            c.set_theta(th)
            c.set_prior(mu)
            c.set_a_mat(th)
        batch = lone[0].svmpc_batch(B, seeds=[3 + b for b in range(B)])

        def tick_batch():
            batch.tick(states, 1, params=params)

        def tick_lone():
            for b, c in enumerate(lone):
                c.svmpc_tick(states[b], 1, params=None if params is None else params[b])

        nb, nl = ticks_for(tick_batch), ticks_for(tick_lone)
        tb, tl = [], []
        for _ in range(REPS):  # alternating: both legs see the same neighbours on the host and the device
            tb.append(leg(tick_batch, nb))
            tl.append(leg(tick_lone, nl))
        mb, ml = float(np.median(tb)), float(np.median(tl))
        print("%5s %3d  %10.0f [%10.0f %10.0f]  %10.0f [%10.0f %10.0f]  %9.1f %9.1f  %6.2f"
              % (name, B, B / mb, B / max(tb), B / min(tb), B / ml, B / max(tl), B / min(tl), 1e6 * mb, 1e6 * ml, ml / mb), flush=True)
        batch.ctx.profile(True)  # the kernel's own time from the profile counter (one HIP-event pair per launch), after the end-to-end legs
        for _ in range(20):
            tick_batch()
        (ms, n), = batch.ctx.profile_get().values()
        print("            kernel: one batched launch %8.1f us" % (1e3 * ms / n), flush=True)
        batch.close()
        for c in lone:
            c.close()
