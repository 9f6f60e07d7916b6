"""DuSt-MPC episodes on the device against the period-by-period loop they replace.  Device-drawn noise, one SVGD step per period, at the
demo shape (demo/pendulum_config.yaml: Pendulum, N 3, S 128, M 8 over (length, mass), H 30; 256 filter particles, 20 filter steps per
update, Silverman's bandwidth), B in {1, 4, 16, 64, 256}, every plant with its own true (length, mass):
  (a) ONE dust_svmpc_dual_batch_episode of T periods: per period the filters' update, the tick, the plant step and the records on the
      device, queued on one stream; one copy back;
  (b) the loop it replaces, T times: dust_svmpc_dual_batch_tick (states and the previous actions in, action sequences out, the stream
      synchronised), then the B plants stepped on the host by one vectorised numpy step.
Both legs run in the same process on the same library build, alternating, REPS times each after a warm-up; a leg's time is a host clock
around whole episodes (each ends in a device synchronise).  T = 1 is the control: an episode of one period has nothing to save.
Printed: the median environment-periods/s of each leg, the spread (min .. max over the repeats), the ratio of the medians, and - from the
profile counter DUST_K_SVMPC_BATCH, one HIP-event pair per launch, in a pass of its own after the timed legs - the tick kernel's time
per period in either leg (the filters' kernels are not among the profile counters).
    python tools/svmpc_dual_episode_time.py [seconds per window, default 1.0] [largest B, default 256] [periods, default 64,1]"""
import math, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from dust_amd import Context, MpfContext

WINDOW = float(sys.argv[1]) if len(sys.argv) > 1 else 1.0
BMAX = int(sys.argv[2]) if len(sys.argv) > 2 else 256
PERIODS = [int(v) for v in (sys.argv[3] if len(sys.argv) > 3 else "64,1").split(",")]
REPS = 5
N, S, M, H, MP, MPF_STEPS = 3, 128, 8, 30, 256, 20


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


def pair(B, rng):
    """a controller batch and a filter batch of B environments at the demo shape"""
    kw = dict(model="pendulum", kernel="K1", lr=2.0, sigma_a=2.0, sigma_p=2.0, N=N, S=S, M=M, H=H, uncertain_params=("length", "mass"))
    mu = rng.standard_normal((N, H, 1)).astype(np.float32)
    th = (mu + 2 * rng.standard_normal((N, H, 1))).astype(np.float32)
    proto = Context(seed=3, **kw)
    proto.set_theta(th)
    proto.set_prior(mu)
    proto.set_a_mat(th)
    sb = proto.svmpc_batch(B, seeds=[3 + b for b in range(B)])
    proto.close()
    x0 = (1.0 + 0.1 * rng.standard_normal((B, MP, 2))).astype(np.float32)
    m = MpfContext(x0[0], np.array([3.0, 0.0], np.float32), model="pendulum", uncertain_params=("length", "mass"), obs_std=0.1, lr=1e-3, init_bw=0.1)
    mb = m.batch(B)
    m.close()
    mb.set_particles(x0)
    return sb, mb


print("%d repeats per leg, windows of %.1f s" % (REPS, WINDOW))
print("T B episode_env_periods_per_s [min max] loop_env_periods_per_s [min max] episode_us_per_period loop_us_per_period ratio", flush=True)
for T in PERIODS:
    for B in (1, 4, 16, 64, 256):
        if B > BMAX:
            continue
        rng = np.random.default_rng(S + B)
        states = (np.array([3.0, 0.0], np.float32) + 0.1 * rng.standard_normal((B, 2))).astype(np.float32)
        true = rng.uniform(0.8, 1.2, (B, 2)).astype(np.float32)
        c0, c1 = (-3.0 * 9.8 / (2.0 * true[:, 0])).astype(np.float32), (3.0 / (true[:, 1] * true[:, 0] ** 2)).astype(np.float32)

        def step(x, a):  # pendulum.py:82-100 for B plants at once
            u = np.clip(a[:, 0], -2.0, 2.0)
            thd = np.clip(x[:, 1] + np.float32(0.05) * (c0 * np.sin(x[:, 0] + np.float32(math.pi)) + c1 * u), -8.0, 8.0)
            return np.stack((x[:, 0] + thd * np.float32(0.05), thd), 1).astype(np.float32)

        (sb_e, mb_e), (sb_l, mb_l) = pair(B, np.random.default_rng(B)), pair(B, np.random.default_rng(B))
        mb_e.set_obs(states)
        mb_l.set_obs(states)
        keys = (np.arange(B, dtype=np.uint64)[None] << np.uint64(32)) + np.arange(1, T + 1, dtype=np.uint64)[:, None]

        def run_episode():
            sb_e.dual_episode(mb_e, states, T, 1, None, mpf_steps=MPF_STEPS, seeds=keys, plant_params=true, want_pw=False)

        def run_loop():
            x, a = states, None
            for t in range(T):
                a_seq, _, _, _ = sb_l.dual_tick(mb_l, x, a, n_steps=1, mpf_steps=MPF_STEPS, seeds=keys[t])
                a = a_seq[:, 0]
                x = step(x, a)

        ne, nl = episodes_for(run_episode), episodes_for(run_loop)
        te, tl = [], []
        for _ in range(REPS):  # alternating: both legs see the same neighbours on the host and the device
            te.append(leg(run_episode, ne) / T)
            tl.append(leg(run_loop, nl) / T)
        me, ml = float(np.median(te)), float(np.median(tl))
        print("%3d %3d  %10.0f [%10.0f %10.0f]  %10.0f [%10.0f %10.0f]  %9.1f %9.1f  %6.2f"
              % (T, B, B / me, B / max(te), B / min(te), B / ml, B / max(tl), B / min(tl), 1e6 * me, 1e6 * ml, ml / me), flush=True)
        kt = []
        for b, fn in ((sb_e, run_episode), (sb_l, run_loop)):  # the tick kernel's own time: one launch per period in both legs
            b.ctx.profile(True)
            for _ in range(3):
                fn()
            (ms, n), = b.ctx.profile_get().values()
            assert n == 3 * T
            kt.append(1e3 * ms / n)
        for h in (sb_e, mb_e, sb_l, mb_l):
            h.close()
        print("            tick kernel time per period: episode %8.1f us, loop %8.1f us (%.0f %% of the loop's period)"
              % (kt[0], kt[1], 100.0 * kt[1] / (1e6 * ml)), flush=True)
