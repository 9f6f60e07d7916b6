"""Closed-loop environment-periods per second of the dual loop over B plants, two legs in the same process on the same device:
  (a) ONE BatchDualAMPPI of B environments: a period of all of them is one C call (dust_amppi_dual_batch_tick);
  (b) B lone DualAMPPI(fused=True) objects stepped one after the other: B C calls per period, each with its own filter launches, its
      4-byte bandwidth round trip and its synchronisations.
Scenario: examples/amppi_dual_batch_example.py - Pendulum (length, mass), S = 1024, H = 20, params_sampling="extended", 256 filter
particles, 20 filter steps, Silverman bandwidths, numpy pendulums with their own true parameters as plants - at B in {1, 4, 16, 64, 256}.  A period
ends with every environment's action on the host (the plants need it), so every timed window ends synchronised.  Both legs are warmed up
(contexts, code objects, the first filter update), then timed REPS times each, alternating; printed: the median environment-periods/s of
each leg, the spread (min .. max over the repeats) and the ratio of the medians.  At B = 1 the batch runs the single-workgroup filter
kernel where a lone object takes the data-polled grid, so the batch is expected to lose at small B.

    python tools/amppi_dual_batch_time.py [seconds per window, default 1.0] [largest B, default 256]"""
import importlib.util
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

WINDOW = float(sys.argv[1]) if len(sys.argv) > 1 else 1.0
BMAX = int(sys.argv[2]) if len(sys.argv) > 2 else 256
REPS, WARM = 5, 5
KW = dict(samples=1024, horizon=20, mpf_particles=256, seed=0, mpf_bw=None, mpf_steps=20)


def example():
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples", "amppi_dual_batch_example.py")
    spec = importlib.util.spec_from_file_location("amppi_dual_batch_example", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def pendulum(states, actions, length, mass, dt=0.05, g=9.8, max_torque=2.0, max_speed=8.0):
    """the plants: rows of (theta, theta_dot) under each row's own length and mass, vectorised over the rows - the batched leg steps all
    its plants in one call, a lone object its own row (the same elementwise operations)"""
    x, u = np.asarray(states, np.float32).reshape(-1, 2), np.clip(np.asarray(actions, np.float32).reshape(-1), -max_torque, max_torque)
    thd = x[:, 1] + dt * (-3.0 * g / (2.0 * length) * np.sin(x[:, 0] + np.pi) + 3.0 / (mass * length ** 2) * u)
    thd = np.clip(thd, -max_speed, max_speed)
    return torch.from_numpy(np.stack([x[:, 0] + thd * dt, thd], 1).astype(np.float32))


def window(period, state, n):
    t0 = time.perf_counter()
    for _ in range(n):
        state = period(state)  # (the actions came to the host inside: the streams are drained)
    return (time.perf_counter() - t0) / n, state


def main():
    ex = example()
    print("B batch_env_periods_per_s [min max] lone_env_periods_per_s [min max] batch_us_per_period lone_us_per_period ratio", flush=True)
    for B in (1, 4, 16, 64, 256):
        if B > BMAX:
            break
        loop, _, start, (length, mass) = ex.scenario(n_envs=B, **KW)
        lones = [ex.lone(b, n_envs=B, **KW) for b in range(B)]
        length, mass = length.numpy().astype(np.float64), mass.numpy().astype(np.float64)
        plants = [lambda x, u, b=b: pendulum(x, u, length[b:b + 1], mass[b:b + 1]) for b in range(B)]

        def period_batch(states):
            return loop.tick(states, lambda x, u: pendulum(x, u, length, mass))[1]

        def period_lone(states):
            return [lo.tick(s, pl)[1] for (lo, _, _), pl, s in zip(lones, plants, states)]

        sb, sl = start.clone(), [s.reshape(1, -1) for _, _, s in lones]
        _, sb = window(period_batch, sb, WARM)
        _, sl = window(period_lone, sl, WARM)
        pb, sb = window(period_batch, sb, 3)
        pl, sl = window(period_lone, sl, 3)
        nb, nl = max(3, int(WINDOW / pb)), max(3, int(WINDOW / pl))
        tb, tl = [], []
        for _ in range(REPS):  # alternating: both legs see the same neighbours on the host and the device
            t, sb = window(period_batch, sb, nb)
            tb.append(t)
            t, sl = window(period_lone, sl, nl)
            tl.append(t)
        ok = bool(torch.isfinite(sb).all()) and all(bool(torch.isfinite(s).all()) for s in sl)
        mb, ml = float(np.median(tb)), float(np.median(tl))
        print("%3d  %9.0f [%9.0f %9.0f]  %9.0f [%9.0f %9.0f]  %10.1f %10.1f  %6.2f%s"
              % (B, B / mb, B / max(tb), B / min(tb), B / ml, B / max(tl), B / min(tl), 1e6 * mb, 1e6 * ml, ml / mb, "" if ok else "  NON-FINITE STATE"), flush=True)
        loop.controller._batch.close()
        loop._mb.close()
        for lo, _, _ in lones:
            lo.controller._ctx.close()
            lo.mpf._dev.close()


if __name__ == "__main__":
    main()
