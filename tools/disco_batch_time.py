"""MultiDISCO over a batch of plants against what it replaces, at the shapes of the reference's demo/pendulum_example.py:217-261 (Pendulum,
S 128, H 30, device-drawn noise): `mppi` (N 1, no parameters: the MPPI baseline), `disco` (N 1, the 5 sigma points of (length, mass)) and
`n4` (N 4, M 4 sampled rows).  B in {1, 4, 16, 64, 256}.
  tick     (a) ONE dust_disco_batch_tick (forward + step("average"), next actions back, the stream synchronised) against
           (b) B lone contexts in turn: dust_disco_forward + dust_disco_step each (the lone pair's launches and round trips);
  episode  (a) ONE dust_disco_batch_episode of T periods (forward, step, plant step and records on the device, one copy back) against
           (b) the loop it replaces, T times: dust_disco_batch_tick, then the B plants stepped on the host by one vectorised numpy step.
           T = 1 is the control: an episode of one period is a tick plus the plant.
The legs of a pair run in the same process, alternating, REPS times each after a warm-up; a leg's time is a host clock around whole calls
(every call ends synchronised: its outputs are read back).  Printed: the median environment-ticks/s of each leg, the spread (min .. max
over the repeats) and the ratio of the medians.
    python tools/disco_batch_time.py [seconds per window, default 0.5] [largest B, default 256] [periods per episode, default 64] [shapes]"""
import math, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from dust_amd import Context

WINDOW = float(sys.argv[1]) if len(sys.argv) > 1 else 0.5
BMAX = int(sys.argv[2]) if len(sys.argv) > 2 else 256
T = int(sys.argv[3]) if len(sys.argv) > 3 else 64
REPS = 5
SHAPES = {"mppi": dict(N=1, M=1, up=None, sigma=False), "disco": dict(N=1, M=5, up=("length", "mass"), sigma=True),
          "n4": dict(N=4, M=4, up=("length", "mass"), sigma=False)}
ONLY = sys.argv[4].split(",") if len(sys.argv) > 4 else list(SHAPES)
S, H = 128, 30


def leg(fn, n):
    t0 = time.perf_counter()
    for _ in range(n):
        fn()
    return (time.perf_counter() - t0) / n


def calls_for(fn):
    """calls per timed window: warm the leg up, then size the window from a short probe"""
    for _ in range(3):
        fn()
    return max(2, int(WINDOW / leg(fn, 2)) + 1)


def pair(a, b, per_call):
    """alternating legs -> (median seconds per unit of a, of b, their min / max)"""
    na, nb = calls_for(a), calls_for(b)
    ta, tb = [], []
    for _ in range(REPS):  # alternating: both legs see the same neighbours on the host and the device
        ta.append(leg(a, na) / per_call)
        tb.append(leg(b, nb) / per_call)
    return float(np.median(ta)), float(np.median(tb)), ta, tb


def proto_of(shape, seed):
    kw = dict(model="pendulum", N=shape["N"], S=S, M=shape["M"], H=H, temperature=1.0, alpha=1.0, sigma_a=2.0, seed=seed)
    if shape["up"]:
        kw.update(uncertain_params=shape["up"], sampling=True)
    c = Context(**kw)
    if shape["sigma"]:  # MerweScaledUTF(n=2, alpha=0.5): lambda + n = 0.5
        c.set_param_weights(np.array([-3.0, 1.0, 1.0, 1.0, 1.0], np.float32))
        c.set_sigma_scale(0.5)
    return c


print("S = %d, H = %d, T = %d periods per episode, %d repeats per leg" % (S, H, T, REPS))
print("what shape B batch_env_ticks_per_s [min max] replaced_env_ticks_per_s [min max] batch_us replaced_us ratio", flush=True)
for name, shape in SHAPES.items():
    if name not in ONLY:
        continue
    for B in (1, 4, 16, 64, 256):
        if B > BMAX:
            continue
        N, M = shape["N"], shape["M"]
        rng = np.random.default_rng(S + B)
        states = (np.array([3.0, 0.0], np.float32) + 0.1 * rng.standard_normal((B, 2))).astype(np.float32)
        params = true = None
        if shape["up"]:
            params = (1.0 + 0.1 * rng.standard_normal((B, M, 2))).astype(np.float32)
            true = rng.uniform(0.8, 1.2, (B, 2)).astype(np.float32)
        ln, ms = (true[:, 0], true[:, 1]) if true is not None else (np.ones(B, np.float32), np.ones(B, np.float32))
        c0, c1 = (-3.0 * 9.8 / (2.0 * ln)).astype(np.float32), (3.0 / (ms * ln ** 2)).astype(np.float32)

        def step(x, a):  # pendulum.py:82-100 for B plants at once
            u = np.clip(a[:, 0], -2.0, 2.0)
            thd = np.clip(x[:, 1] + np.float32(0.05) * (c0 * np.sin(x[:, 0] + np.float32(math.pi)) + c1 * u), -8.0, 8.0)
            return np.stack((x[:, 0] + thd * np.float32(0.05), thd), 1).astype(np.float32)

        proto = proto_of(shape, 3)
        batch, in_loop, on_device = (proto.disco_batch(B, seeds=[3 + b for b in range(B)]) for _ in range(3))
        proto.close()
        lone = [proto_of(shape, 3 + b) for b in range(B)]

        def run_tick():
            batch.tick(states, "average", 1, params=params)

        def run_lone():
            for b in range(B):
                lone[b].disco_forward(states[b], None, None if params is None else params[b], want_omega=False)
                lone[b].disco_step("average", 1)

        mb, ml, tb, tl = pair(run_tick, run_lone, 1)
        print("tick    %6s %3d  %10.0f [%10.0f %10.0f]  %10.0f [%10.0f %10.0f]  %9.1f %9.1f  %6.2f"
              % (name, B, B / mb, B / max(tb), B / min(tb), B / ml, B / max(tl), B / min(tl), 1e6 * mb, 1e6 * ml, ml / mb), flush=True)
        for c in lone:
            c.close()
        for periods in (T, 1):
            def run_episode():
                on_device.episode(states, periods, "average", params, true, params_once=params is not None)

            def run_loop():
                x = states
                for _ in range(periods):
                    x = step(x, in_loop.tick(x, "average", 1, params=params)[:, 0])

            me, mo, te, to = pair(run_episode, run_loop, periods)
            print("episode%-2s%5s %3d  %10.0f [%10.0f %10.0f]  %10.0f [%10.0f %10.0f]  %9.1f %9.1f  %6.2f"
                  % ("" if periods > 1 else "1", name, B, B / me, B / max(te), B / min(te), B / mo, B / max(to), B / min(to), 1e6 * me, 1e6 * mo, mo / me),
                  flush=True)
        for b in (batch, in_loop, on_device):
            b.close()
