"""The batched AMPPI tick against the same work done serially: Pendulum, H = 30, S in {1024, 8192}, B in {1, 4, 16, 64, 256}, device-drawn
noise, the model's own parameters (no host rows: neither leg uploads anything but the plant states), nothing read back.
  (a) ONE dust_amppi_batch_update of B environments per period;
  (b) B lone dust_amppi_update calls per period, enqueued back to back on B contexts (each on its own stream).
Both legs run in the same process, alternating, REPS times each after a warm-up of every shape; a leg's time is a host clock around
`ticks` periods that end in a synchronisation of every stream used.  Printed: the median environment-ticks/s of each leg, the spread
(min .. max over the repeats) and the ratio of the medians.
    python tools/amppi_batch_time.py [seconds per leg, default 0.3]"""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from dust_amd import Context

WINDOW = float(sys.argv[1]) if len(sys.argv) > 1 else 0.3
H, LAM, SIGMA, REPS = 30, 100.0, 2.0, 5


def leg(fn, sync, ticks):
    sync()
    t0 = time.perf_counter()
    for _ in range(ticks):
        fn()
    sync()
    return (time.perf_counter() - t0) / ticks


def ticks_for(fn, sync):
    """periods per timed window: warm the shape up, then size the window from a short probe"""
    for _ in range(10):
        fn()
    per = leg(fn, sync, 10)
    return max(10, int(WINDOW / per))


print("S B batch_env_ticks_per_s [min max] lone_env_ticks_per_s [min max] batch_us_per_period lone_us_per_period ratio", flush=True)
for S in (1024, 8192):
    for B in (1, 4, 16, 64, 256):
        rng = np.random.default_rng(S + B)
        a0 = (0.5 * rng.standard_normal((H, 1))).astype(np.float32)
        states = (np.array([3.0, 0.0], np.float32) + 0.1 * rng.standard_normal((B, 2))).astype(np.float32)
        kw = dict(model="pendulum", N=1, S=S, M=1, H=H, temperature=LAM, alpha=1.0 / LAM, sigma_a=SIGMA)
        lone = [Context(seed=3 + b, **kw) for b in range(B)]
        for c in lone:
            c.set_a_seq(a0)
        batch = lone[0].amppi_batch(B, seeds=[3 + b for b in range(B)])

        def tick_batch():
            batch.update(states, want_outputs=False)

        def tick_lone():
            for b, c in enumerate(lone):
                c.amppi_update(states[b], want_outputs=False)

        def sync_lone():
            for c in lone:
                c.sync()

        nb, nl = ticks_for(tick_batch, batch.ctx.sync), ticks_for(tick_lone, sync_lone)
        tb, tl = [], []
        for _ in range(REPS):  # alternating: both legs see the same neighbours on the host and the device
            tb.append(leg(tick_batch, batch.ctx.sync, nb))
            tl.append(leg(tick_lone, sync_lone, nl))
        mb, ml = float(np.median(tb)), float(np.median(tl))
        print("%5d %3d  %10.0f [%10.0f %10.0f]  %10.0f [%10.0f %10.0f]  %9.1f %9.1f  %6.2f"
              % (S, B, B / mb, B / max(tb), B / min(tb), B / ml, B / max(tl), B / min(tl), 1e6 * mb, 1e6 * ml, ml / mb), flush=True)
        # the kernels' own time from the profile counters (one HIP-event pair per launch), after the end-to-end legs
        kern = []
        for ctx, fn in ((batch.ctx, tick_batch), (lone[0], lambda: lone[0].amppi_update(states[0], want_outputs=False))):
            ctx.profile(True)
            for _ in range(50):
                fn()
            (ms, n), = ctx.profile_get().values()
            ctx.profile(False)
            kern.append(1e3 * ms / n)
        print("            kernel: batched launch %8.1f us, one lone launch %8.1f us" % tuple(kern), flush=True)
        batch.close()
        for c in lone:
            c.close()
