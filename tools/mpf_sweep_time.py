"""What per-environment FILTER hyper-parameters (dust_mpf_batch_set_hyper) cost and save in the DuSt-MPC episode on the device.  One
dust_svmpc_dual_batch_episode of T periods, device-drawn noise, one SVGD step per period, at the demo shape (demo/pendulum_config.yaml:
Pendulum, N 3, S 128, M 8 over (length, mass), H 30; 256 filter particles, 20 filter steps per update), B in {1, 4, 16, 64, 256}, every
plant with its own true (length, mass):
  (a) rows:    B distinct filter rows (lr, obs_std, bw_scale log-uniform; every other environment a fixed bandwidth, the rest Silverman's
               rule) - mpf_silverman_rows_kernel and mpf_optimize_rows_kernel per update;
  (b) no rows: the same pair without rows, Silverman's rule - the uniform kernels, same build, same process;
  (c) in turn: B one-environment pairs, each with its own filter created with environment b's values, one episode each, one after the
               other - what a sweep over the filter's settings costs without rows.
The legs alternate, REPS times each after a warm-up; a leg's time is a host clock around whole episodes (each ends in a device
synchronise).  T = 1 is the control.  Printed: the median environment-periods/s of each leg with its spread (min .. max over the
repeats), rows against no rows, and rows against in turn.
    python tools/mpf_sweep_time.py [seconds per window, default 1.0] [largest B, default 256] [periods, default 64,1]"""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from dust_amd import Context, MpfContext

WINDOW = float(sys.argv[1]) if len(sys.argv) > 1 else 1.0
BMAX = int(sys.argv[2]) if len(sys.argv) > 2 else 256
PERIODS = [int(v) for v in (sys.argv[3] if len(sys.argv) > 3 else "64,1").split(",")]
REPS = 5
N, S, M, H, MP, MPF_STEPS = 3, 128, 8, 30, 256, 20
PROTO = dict(lr=1e-3, obs_std=0.1, bw_scale=1.0)


def leg(fn, n):
    t0 = time.perf_counter()
    for _ in range(n):
        fn()
    return (time.perf_counter() - t0) / n


def episodes_for(fn):
    """episodes per timed window: warm the leg up, then size the window from a short probe"""
    fn()
    return max(1, int(WINDOW / leg(fn, 1)))


def pair(envs, x0, filt=PROTO):
    """a controller batch and a filter batch of the environments `envs` at the demo shape; the filter prototype is created with `filt`"""
    rng = np.random.default_rng(S)
    kw = dict(model="pendulum", kernel="K1", lr=2.0, sigma_a=2.0, sigma_p=2.0, N=N, S=S, M=M, H=H, uncertain_params=("length", "mass"))
    mu = rng.standard_normal((N, H, 1)).astype(np.float32)
    th = (mu + 2 * rng.standard_normal((N, H, 1))).astype(np.float32)
    proto = Context(seed=3, **kw)
    proto.set_theta(th)
    proto.set_prior(mu)
    proto.set_a_mat(th)
    sb = proto.svmpc_batch(len(envs), seeds=[3 + b for b in envs])
    proto.close()
    m = MpfContext(x0[envs[0]], np.array([3.0, 0.0], np.float32), model="pendulum", uncertain_params=("length", "mass"), obs_std=filt["obs_std"],
                   lr=filt["lr"], bw_scale=filt["bw_scale"], init_bw=0.1)
    mb = m.batch(len(envs))
    m.close()
    mb.set_particles(x0[envs])
    return sb, mb


def draw_rows(B, rng):
    lu = lambda lo, hi: float(np.float32(np.exp(rng.uniform(np.log(lo), np.log(hi)))))
    return [dict(lr=lu(3e-4, 3e-3), obs_std=lu(0.05, 0.2), bw_scale=lu(0.5, 2.0), bw=lu(0.05, 0.2) if b % 2 else 0.0) for b in range(B)]


print("%d repeats per leg, windows of %.1f s" % (REPS, WINDOW))
print("T B rows_env_periods_per_s [min max] no_rows [min max] in_turn [min max] rows/no_rows rows/in_turn", flush=True)
for T in PERIODS:
    for B in (1, 4, 16, 64, 256):
        if B > BMAX:
            continue
        rng = np.random.default_rng(S + B)
        states = (np.array([3.0, 0.0], np.float32) + 0.1 * rng.standard_normal((B, 2))).astype(np.float32)
        true = rng.uniform(0.8, 1.2, (B, 2)).astype(np.float32)
        x0 = (1.0 + 0.1 * rng.standard_normal((B, MP, 2))).astype(np.float32)
        rows = draw_rows(B, rng)
        envs = list(range(B))
        sb_r, mb_r = pair(envs, x0)
        sb_u, mb_u = pair(envs, x0)
        mb_r.set_hyper(rows)
        ones = [pair([b], x0, rows[b]) for b in envs]
        for mb in (mb_r, mb_u):
            mb.set_obs(states)
        for b, (_, m1) in enumerate(ones):
            m1.set_obs(states[b:b + 1])
        keys = (np.arange(B, dtype=np.uint64)[None] << np.uint64(32)) + np.arange(1, T + 1, dtype=np.uint64)[:, None]

        def run_rows():
            sb_r.dual_episode(mb_r, states, T, 1, None, mpf_steps=MPF_STEPS, seeds=keys, plant_params=true, want_pw=False)

        def run_uniform():
            sb_u.dual_episode(mb_u, states, T, 1, None, mpf_steps=MPF_STEPS, seeds=keys, plant_params=true, want_pw=False)

        def run_in_turn():
            for b, (s1, m1) in enumerate(ones):
                s1.dual_episode(m1, states[b:b + 1], T, 1, None, mpf_steps=MPF_STEPS, mpf_bw=rows[b]["bw"] if rows[b]["bw"] > 0 else None,
                                seeds=keys[:, b:b + 1], plant_params=true[b:b + 1], want_pw=False)

        legs = (run_rows, run_uniform, run_in_turn)
        ns = [episodes_for(fn) for fn in legs]
        ts = [[], [], []]
        for _ in range(REPS):  # alternating: the legs see the same neighbours on the host and the device
            for k, fn in enumerate(legs):
                ts[k].append(leg(fn, ns[k]) / T)
        med = [float(np.median(t)) for t in ts]
        print("%3d %3d  " % (T, B) + "  ".join("%10.0f [%10.0f %10.0f]" % (B / med[k], B / max(ts[k]), B / min(ts[k])) for k in range(3))
              + "  %6.3f %7.2f" % (med[1] / med[0], med[2] / med[0]), flush=True)
        for h in [sb_r, mb_r, sb_u, mb_u] + [h for p in ones for h in p]:
            h.close()
