"""Dual AMPPI episodes on the device against the tick-per-period loop they replace, two legs in the same process on the same device:
  (a) `BatchDualAMPPI.run_episodes(states, T)`: ONE dust_amppi_dual_batch_episode of T periods - per period the filters' update, the
      tick, the plant's step and the roll queued on one stream, the filters conditioned on the device, one wait per call;
  (b) the loop it replaces, T times: `BatchDualAMPPI.tick` - one dust_amppi_dual_batch_tick with its outputs read back, then the B
      plants stepped on the host by one vectorised numpy step.
Scenario: tools/amppi_dual_batch_time.py's (examples/amppi_dual_batch_example.py) - Pendulum (length, mass), S = 1024, H = 20,
params_sampling="extended", 256 filter particles, 20 filter steps, Silverman bandwidths, every plant under its own true length and mass
- at B in {1, 4, 16, 64, 256}.  Both legs are warmed up, then timed REPS times each, alternating; a leg's time is a host clock around whole
episodes.  T = 1 is run as the control.  Printed: the median environment-periods/s of each leg, the spread (min .. max over the repeats), the ratio of
the medians, and - from the controller batch's profile counters, in a pass of its own with one HIP-event pair and one wait per launch - the
time per period of the controller's kernels in either leg (the period kernel; tick plus roll).  The filters' launches are not counted there.

    python tools/amppi_dual_episode_time.py [seconds per window, default 1.0] [largest B, default 256] [periods per episode, default 64]"""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np
import torch

from amppi_dual_batch_time import KW, example, pendulum

WINDOW = float(sys.argv[1]) if len(sys.argv) > 1 else 1.0
BMAX = int(sys.argv[2]) if len(sys.argv) > 2 else 256
T = int(sys.argv[3]) if len(sys.argv) > 3 else 64
REPS = 5


def leg(fn, state, n):
    t0 = time.perf_counter()
    for _ in range(n):
        state = fn(state)
    return (time.perf_counter() - t0) / n, state


def main():
    ex = example()
    print("%d repeats per leg" % REPS)
    print("B T episode_env_periods_per_s [min max] loop_env_periods_per_s [min max] episode_us_per_period loop_us_per_period ratio "
          "controller_kernel_us_per_period_episode controller_kernel_us_per_period_loop", flush=True)
    for B in (1, 4, 16, 64, 256):
        if B > BMAX:
            break
        on_device, _, start, (length, mass) = ex.scenario(n_envs=B, **KW)
        in_loop = ex.scenario(n_envs=B, **KW)[0]
        true = torch.stack((length, mass), 1).float()
        ln, ms = length.numpy().astype(np.float64), mass.numpy().astype(np.float64)
        se, sl = start.clone(), start.clone()
        for periods in (T, 1):  # (T = 1 is the control: one launch chain and one wait per period in both legs)

            def run_episode(states):
                return on_device.run_episodes(states, periods, plant_params=true)[0][-1]

            def run_loop(states):
                for _ in range(periods):
                    states = in_loop.tick(states, lambda x, u: pendulum(x, u, ln, ms))[1]
                return states

            for _ in range(2):
                se, sl = run_episode(se), run_loop(sl)
            pe, se = leg(run_episode, se, 2)
            pl, sl = leg(run_loop, sl, 2)
            ne, nl = max(2, int(WINDOW / pe) + 1), max(2, int(WINDOW / pl) + 1)
            te, tl = [], []
            for _ in range(REPS):  # alternating: both legs see the same neighbours on the host and the device
                t, se = leg(run_episode, se, ne)
                te.append(t / periods)
                t, sl = leg(run_loop, sl, nl)
                tl.append(t / periods)
            kt = []  # the controller batch's own kernels per period (period kernel / tick + roll); the filters' launches are not counted
            for lp, fn, st in ((on_device, run_episode, se), (in_loop, run_loop, sl)):
                ctx = lp.controller._batch.ctx
                ctx.profile(True)
                for _ in range(3):
                    st = fn(st)
                kt.append(1e3 * sum(v[0] for v in ctx.profile_get().values()) / (3 * periods))
                ctx.profile(False)
                if lp is on_device:
                    se = st
                else:
                    sl = st
            ok = bool(torch.isfinite(se).all()) and bool(torch.isfinite(sl).all())
            me, ml = float(np.median(te)), float(np.median(tl))
            print("%3d %3d  %9.0f [%9.0f %9.0f]  %9.0f [%9.0f %9.0f]  %10.1f %10.1f  %6.2f  %8.1f %8.1f%s"
                  % (B, periods, B / me, B / max(te), B / min(te), B / ml, B / max(tl), B / min(tl), 1e6 * me, 1e6 * ml, ml / me, kt[0], kt[1],
                     "" if ok else "  NON-FINITE STATE"), flush=True)
        for lp in (on_device, in_loop):
            lp.controller._batch.close()
            lp._mb.close()


if __name__ == "__main__":
    main()
