"""The batched SVMPC tick against the same work done serially, closed loop: every period hands the plant states in and reads the chosen
action sequences back.  Device-drawn noise, one SVGD step per tick, at
  demo  - demo/pendulum_config.yaml's shape: Pendulum, N 3, S 128, M 8 (length, mass sampled: [M, 2] rows per tick from the host), H 30;
  cfg1  - BASELINE config 1's shape: Pendulum, N 32, S 128, M 1, H 15;
  skid  - examples/skid_steer_batch_example.py's shape: skid-steer, N 8, S 32, M 4 (x_icr sampled), H 20, the quadratic cost alone;
  skid_nav     - the same with the navigation cost (w_obs 20 on the example's 220 x 220 map, 1513 words: staged into LDS);
  skid_nav_hbm - the same with the map read in place from device memory (DUST_NAV_GRID_HBM=1 while the contexts are created).
B in {1, 4, 16, 64, 256}:
  (a) ONE dust_svmpc_batch_tick of B environments per period;
  (b) B lone dust_svmpc_tick calls per period, B contexts ticked in turn (each on its own stream).
Both legs run in the same process, alternating, REPS times each after a warm-up of every shape; a leg's time is a host clock around
`ticks` periods (every call waits for its outputs).  Printed: the median environment-ticks/s of each leg, the spread (min .. max over
the repeats) and the ratio of the medians.
    python tools/svmpc_batch_time.py [seconds per window, default 1.0] [largest B, default 256] [shapes, comma-separated, default all]"""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from dust_amd import Context

WINDOW = float(sys.argv[1]) if len(sys.argv) > 1 else 1.0
BMAX = int(sys.argv[2]) if len(sys.argv) > 2 else 256
REPS = 3
SKID = dict(family="skid_steer", N=8, S=32, M=4, H=20, uncertain_params=("x_icr",))
SHAPES = {"demo": dict(family="pendulum", N=3, S=128, M=8, H=30, uncertain_params=("length", "mass")),
          "cfg1": dict(family="pendulum", N=32, S=128, M=1, H=15),
          "skid": dict(SKID, w_obs=0.0), "skid_nav": dict(SKID, w_obs=20.0), "skid_nav_hbm": dict(SKID, w_obs=20.0, hbm=True)}
ONLY = sys.argv[3].split(",") if len(sys.argv) > 3 else list(SHAPES)


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


def family_inputs(shape, B, rng):
    """-> (Context keywords, particles' scale and offset, states [B, ds], parameter rows [B, 1, M, P] or None)"""
    N, S, M, H = shape["N"], shape["S"], shape["M"], shape["H"]
    if shape["family"] == "pendulum":
        kw = dict(model="pendulum", kernel="K1", lr=2.0, sigma_a=2.0, sigma_p=2.0, N=N, S=S, M=M, H=H, uncertain_params=shape.get("uncertain_params"))
        states = (np.array([3.0, 0.0], np.float32) + 0.1 * rng.standard_normal((B, 2))).astype(np.float32)
        params = (1.0 + 0.1 * rng.standard_normal((B, 1, M, 2))).astype(np.float32) if M > 1 else None
        return kw, (1.0, 0.0, 1), states, params
    from dust_amd.utils.obstacle_map import generate_obstacle_map, get_obst_preset

    kw = dict(model="skid_steer", kernel="K1", lr=0.5, alpha=0.2, temperature=5.0, sigma_a=1.0, sigma_p=1.0, N=N, S=S, M=M, H=H, dt=0.1,
              uncertain_params=shape["uncertain_params"], min_a=-3.0, max_a=3.0, goal=(2.6, 2.9, 0.0, 0.0, 0.0), w_quad_state=(1.0, 1.0, 0.0, 0.0, 0.0),
              w_quad_term=(20.0, 20.0, 0.0, 0.0, 0.0), w_quad_ctrl=(0.01, 0.01), w_obs=shape["w_obs"], cell_size=0.1)
    if shape["w_obs"] != 0.0:
        m = generate_obstacle_map(map_dim=(22, 22), obst_list=get_obst_preset("grid_6x6", obst_width=1.0), cell_size=0.1, map_type="direct")
        kw["grid"] = np.ascontiguousarray(np.asarray(m.map, np.float32))
    states = (np.array([-2.9, -2.6, 0.6, 0.0, 0.0], np.float32) + 0.1 * rng.standard_normal((B, 5))).astype(np.float32)
    params = rng.uniform(0.15, 0.35, (B, 1, M, 1)).astype(np.float32)
    return kw, (0.5, 1.5, 2), states, params


print("shape B batch_env_ticks_per_s [min max] lone_env_ticks_per_s [min max] batch_us_per_period lone_us_per_period ratio", flush=True)
for name, shape in SHAPES.items():
    if name not in ONLY:
        continue
    for B in (1, 4, 16, 64, 256):
        if B > BMAX:
            continue
        N, H = shape["N"], shape["H"]
        rng = np.random.default_rng(shape["S"] + B)
        kw, (scale, off, da), states, params = family_inputs(shape, B, rng)
        mu = (off + scale * rng.standard_normal((N, H, da))).astype(np.float32)
        th = (mu + 2 * scale * rng.standard_normal((N, H, da))).astype(np.float32)
        if shape.get("hbm"):  # (a development switch, read when a context is created: the batch's inner context is one)
            os.environ["DUST_NAV_GRID_HBM"] = "1"
        lone = [Context(seed=3 + b, **kw) for b in range(B)]
        for c in lone:
            c.set_theta(th)
            c.set_prior(mu)
            c.set_a_mat(th)
        batch = lone[0].svmpc_batch(B, seeds=[3 + b for b in range(B)])
        os.environ.pop("DUST_NAV_GRID_HBM", None)

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
        print("%12s %3d  %10.0f [%10.0f %10.0f]  %10.0f [%10.0f %10.0f]  %9.1f %9.1f  %6.2f"
              % (name, B, B / mb, B / max(tb), B / min(tb), B / ml, B / max(tl), B / min(tl), 1e6 * mb, 1e6 * ml, ml / mb), flush=True)
        batch.ctx.profile(True)  # the kernel's own time from the profile counter (one HIP-event pair per launch), after the end-to-end legs
        for _ in range(20):
            tick_batch()
        (ms, n), = batch.ctx.profile_get().values()
        print("            kernel: one batched launch %8.1f us" % (1e3 * ms / n), flush=True)
        batch.close()
        for c in lone:
            c.close()
