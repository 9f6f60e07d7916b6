"""Closed-loop episodes on the device against the host loop they replace.  Device-drawn noise, one SVGD step per period, T periods per
episode, at
  demo - demo/pendulum_config.yaml's shape: Pendulum, N 3, S 128, M 8 (length, mass sampled), H 30;
  skid - tools/svmpc_batch_time.py's skid-steer shape: N 8, S 32, M 4 (x_icr sampled), H 20, the quadratic cost alone.
B in {1, 4, 16, 64, 256}:
  (a) ONE dust_svmpc_batch_episode of T periods: tick, plant step and records on the device, one copy back;
  (b) the loop it replaces, T times: dust_svmpc_batch_tick (states in, action sequences out, the stream synchronised), then the B
      plants stepped on the host by one vectorised numpy step.
Both legs run in the same process, alternating, REPS times each after a warm-up; a leg's time is a host clock around whole episodes.
Printed: the median environment-ticks/s of each leg, the spread (min .. max over the repeats), the ratio of the medians, and - from the
profile counter, one HIP-event pair per launch, in a pass of its own after the timed legs - the kernel time per period of either leg, so
that the share of a period that is round trip rather than tick can be read off.
    python tools/svmpc_episode_time.py [seconds per window, default 1.0] [largest B, default 256] [periods per episode, default 64] [shapes]"""
import math, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from dust_amd import Context

WINDOW = float(sys.argv[1]) if len(sys.argv) > 1 else 1.0
BMAX = int(sys.argv[2]) if len(sys.argv) > 2 else 256
T = int(sys.argv[3]) if len(sys.argv) > 3 else 64
REPS = 5
SHAPES = {"demo": dict(family="pendulum", N=3, S=128, M=8, H=30, uncertain_params=("length", "mass")),
          "skid": dict(family="skid_steer", N=8, S=32, M=4, H=20, uncertain_params=("x_icr",))}
ONLY = sys.argv[4].split(",") if len(sys.argv) > 4 else list(SHAPES)
SKID_DT, SKID_WR, SKID_AD = 0.1, 0.1, 0.5  # skid-steer: the step below reads x_icr from the true row, these from here


def family_inputs(shape, B, rng):
    """-> (Context keywords, particles' (scale, offset, da), states [B, ds], rows [B, 1, M, P] of one period, true rows [B, P], host step)"""
    N, S, M, H = shape["N"], shape["S"], shape["M"], shape["H"]
    if shape["family"] == "pendulum":
        kw = dict(model="pendulum", kernel="K1", lr=2.0, sigma_a=2.0, sigma_p=2.0, N=N, S=S, M=M, H=H, uncertain_params=shape["uncertain_params"])
        states = (np.array([3.0, 0.0], np.float32) + 0.1 * rng.standard_normal((B, 2))).astype(np.float32)
        params = (1.0 + 0.1 * rng.standard_normal((B, 1, M, 2))).astype(np.float32)
        true = rng.uniform(0.8, 1.2, (B, 2)).astype(np.float32)
        c0, c1 = (-3.0 * 9.8 / (2.0 * true[:, 0])).astype(np.float32), (3.0 / (true[:, 1] * true[:, 0] ** 2)).astype(np.float32)

        def step(x, a):  # pendulum.py:82-100 for B plants at once
            u = np.clip(a[:, 0], -2.0, 2.0)
            thd = np.clip(x[:, 1] + np.float32(0.05) * (c0 * np.sin(x[:, 0] + np.float32(math.pi)) + c1 * u), -8.0, 8.0)
            return np.stack((x[:, 0] + thd * np.float32(0.05), thd), 1).astype(np.float32)

        return kw, (1.0, 0.0, 1), states, params, true, step
    kw = dict(model="skid_steer", kernel="K1", lr=0.5, alpha=0.2, temperature=5.0, sigma_a=1.0, sigma_p=1.0, N=N, S=S, M=M, H=H, dt=SKID_DT,
              uncertain_params=shape["uncertain_params"], min_a=-3.0, max_a=3.0, goal=(2.6, 2.9, 0.0, 0.0, 0.0), w_quad_state=(1.0, 1.0, 0.0, 0.0, 0.0),
              w_quad_term=(20.0, 20.0, 0.0, 0.0, 0.0), w_quad_ctrl=(0.01, 0.01), w_obs=0.0, cell_size=0.1, wheel_radius=SKID_WR, axial_distance=SKID_AD)
    states = (np.array([-2.9, -2.6, 0.6, 0.0, 0.0], np.float32) + 0.1 * rng.standard_normal((B, 5))).astype(np.float32)
    params = rng.uniform(0.15, 0.35, (B, 1, M, 1)).astype(np.float32)
    true = rng.uniform(0.15, 0.35, (B, 1)).astype(np.float32)

    def step(x, a):  # skid_steer_robot.py:84-122 for B plants at once
        r, l = np.clip(a[:, 0], -3.0, 3.0), np.clip(a[:, 1], -3.0, 3.0)
        lin, ang = (r + l) * np.float32(math.pi * SKID_WR), (r - l) * np.float32(2 * math.pi * SKID_WR / SKID_AD)
        fwd, lat = lin * np.float32(SKID_DT), -ang * true[:, 0] * np.float32(SKID_DT)
        c, s = np.cos(x[:, 2]), np.sin(x[:, 2])
        return np.stack((x[:, 0] + fwd * c - lat * s, x[:, 1] + fwd * s + lat * c, x[:, 2] + ang * np.float32(SKID_DT), lin, ang), 1).astype(np.float32)

    return kw, (0.5, 1.5, 2), states, params, true, step


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


print("T = %d periods per episode, %d repeats per leg" % (T, REPS))
print("shape B episode_env_ticks_per_s [min max] loop_env_ticks_per_s [min max] episode_us_per_period loop_us_per_period ratio", flush=True)
for name, shape in SHAPES.items():
    if name not in ONLY:
        continue
    for B in (1, 4, 16, 64, 256):
        if B > BMAX:
            continue
        N, H = shape["N"], shape["H"]
        rng = np.random.default_rng(shape["S"] + B)
        kw, (scale, off, da), states, params, true, step = family_inputs(shape, B, rng)
        mu = (off + scale * rng.standard_normal((N, H, da))).astype(np.float32)
        th = (mu + 2 * scale * rng.standard_normal((N, H, da))).astype(np.float32)
        proto = Context(seed=3, **kw)
        proto.set_theta(th)
        proto.set_prior(mu)
        proto.set_a_mat(th)
        on_device, in_loop = proto.svmpc_batch(B, seeds=[3 + b for b in range(B)]), proto.svmpc_batch(B, seeds=[3 + b for b in range(B)])
        proto.close()
        params_T = np.ascontiguousarray(np.broadcast_to(params[None], (T,) + params.shape))

        def run_episode():
            on_device.episode(states, T, 1, params_T, true, want_pw=False)

        def run_loop():
            x = states
            for _ in range(T):
                a_seq, _ = in_loop.tick(x, 1, params=params)
                x = step(x, a_seq[:, 0])

        ne, nl = episodes_for(run_episode), episodes_for(run_loop)
        te, tl = [], []
        for _ in range(REPS):  # alternating: both legs see the same neighbours on the host and the device
            te.append(leg(run_episode, ne) / T)
            tl.append(leg(run_loop, nl) / T)
        me, ml = float(np.median(te)), float(np.median(tl))
        print("%6s %3d  %10.0f [%10.0f %10.0f]  %10.0f [%10.0f %10.0f]  %9.1f %9.1f  %6.2f"
              % (name, B, B / me, B / max(te), B / min(te), B / ml, B / max(tl), B / min(tl), 1e6 * me, 1e6 * ml, ml / me), flush=True)
        kt = []
        for b, fn in ((on_device, run_episode), (in_loop, run_loop)):  # the kernels' own time: T periods per launch / one period per launch
            b.ctx.profile(True)
            for _ in range(3):
                fn()
            (ms, n), = b.ctx.profile_get().values()
            kt.append(1e3 * ms / (3 * T))
            b.close()
        print("            kernel time per period: episode %8.1f us, loop %8.1f us (%.0f %% of the loop's period)"
              % (kt[0], kt[1], 100.0 * kt[1] / (1e6 * ml)), flush=True)
