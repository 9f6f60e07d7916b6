"""Closed-loop AMPPI episodes on the device against the host loop they replace.  Pendulum, H = 30, no parameter sampling ("none"),
device-drawn noise, S in {1 024, 8 192}, B in {1, 4, 16, 64, 256}, T periods per episode (and T = 1 as the control):
  (a) ONE dust_amppi_batch_episode of T periods: per period one launch - tick, plant step, records, roll - and one copy back per call;
  (b) the loop it replaces, T times: dust_amppi_batch_update with a_seq read back (the stream synchronised), the B plants stepped on
      the host by one vectorised numpy step, dust_amppi_batch_roll.
Both legs run in the same process, alternating, REPS times each after a warm-up; a leg's time is a host clock around whole episodes.
Printed: the median environment-periods/s of each leg, the spread (min .. max over the repeats), the ratio of the medians, and - from the
profile counters, one HIP-event pair per launch, in a pass of its own after the timed legs - the kernel time per period of either leg
(the loop's: update plus roll).
    python tools/amppi_episode_time.py [seconds per window, default 1.0] [largest B, default 256] [periods, default 64] [S list, default 1024,8192]"""
import math, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from dust_amd import Context

WINDOW = float(sys.argv[1]) if len(sys.argv) > 1 else 1.0
BMAX = int(sys.argv[2]) if len(sys.argv) > 2 else 256
T = int(sys.argv[3]) if len(sys.argv) > 3 else 64
SIZES = [int(v) for v in sys.argv[4].split(",")] if len(sys.argv) > 4 else [1024, 8192]
REPS = 5
H, DT = 30, 0.05
C0, C1 = np.float32(-3.0 * 9.8 / 2.0), np.float32(3.0)  # the nominal pendulum: g 9.8, mass 1, length 1


def step(x, a):  # pendulum.py:82-100 for B plants at once
    u = np.clip(a[:, 0], -2.0, 2.0)
    thd = np.clip(x[:, 1] + np.float32(DT) * (C0 * np.sin(x[:, 0] + np.float32(math.pi)) + C1 * u), -8.0, 8.0)
    return np.stack((x[:, 0] + thd * np.float32(DT), thd), 1).astype(np.float32)


def leg(fn, n):
    t0 = time.perf_counter()
    for _ in range(n):
        fn()
    return (time.perf_counter() - t0) / n


def episodes_for(fn):
    """episodes per timed window: warm the leg up, then size the window from a short probe"""
    for _ in range(3):
        fn()
    return max(2, int(WINDOW / leg(fn, 2)) + 1)


print("%d repeats per leg" % REPS)
print("S B T episode_env_periods_per_s [min max] loop_env_periods_per_s [min max] episode_us_per_period loop_us_per_period ratio "
      "kernel_us_per_period_episode kernel_us_per_period_loop", flush=True)
for S in SIZES:
    for B in (1, 4, 16, 64, 256):
        if B > BMAX:
            continue
        rng = np.random.default_rng(S + B)
        states = (np.array([3.0, 0.0], np.float32) + 0.1 * rng.standard_normal((B, 2))).astype(np.float32)
        a0 = (0.5 * rng.standard_normal((B, H, 1))).astype(np.float32)
        proto = Context(model="pendulum", N=1, S=S, M=1, H=H, dt=DT, temperature=100.0, alpha=0.01, a_cov=4.0 * np.eye(1, dtype=np.float32),
                        min_a=(-2.0,), max_a=(2.0,), sampling=False, seed=3)
        on_device, in_loop = (proto.amppi_batch(B, [3 + b for b in range(B)]) for _ in range(2))
        proto.close()
        on_device.set_a_seq(a0)
        in_loop.set_a_seq(a0)
        for periods in (T, 1):

            def run_episode():
                on_device.episode(states, periods, want_costs=False)

            def run_loop():
                x = states
                for _ in range(periods):
                    _, _, a_seq, _ = in_loop.update(x, want_costs=False)  # a_seq alone comes back, as the episode records no costs
                    x = step(x, a_seq[:, 0])
                    in_loop.roll(1)

            ne, nl = episodes_for(run_episode), episodes_for(run_loop)
            te, tl = [], []
            for _ in range(REPS):  # alternating: both legs see the same neighbours on the host and the device
                te.append(leg(run_episode, ne) / periods)
                tl.append(leg(run_loop, nl) / periods)
            me, ml = float(np.median(te)), float(np.median(tl))
            kt = []
            for b, fn in ((on_device, run_episode), (in_loop, run_loop)):  # the kernels' own time per period
                b.ctx.profile(True)
                for _ in range(3):
                    fn()
                kt.append(1e3 * sum(ms for ms, _ in b.ctx.profile_get().values()) / (3 * periods))
                b.ctx.profile(False)
            print("%5d %3d %3d  %10.0f [%10.0f %10.0f]  %10.0f [%10.0f %10.0f]  %9.1f %9.1f  %6.2f  %8.1f %8.1f"
                  % (S, B, periods, B / me, B / max(te), B / min(te), B / ml, B / max(tl), B / min(tl), 1e6 * me, 1e6 * ml, ml / me, kt[0], kt[1]),
                  flush=True)
        on_device.close()
        in_loop.close()
