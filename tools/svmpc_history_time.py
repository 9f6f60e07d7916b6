"""What recording the posterior's history costs (dust_svmpc_batch_set_history), and what it replaces.  One dust_svmpc_dual_batch_simulate of
T periods at the demo shape (demo/pendulum_config.yaml: Pendulum, N 3, S 128, M 8 over (length, mass), H 30; 256 filter particles, 20
filter steps per update, Silverman's bandwidth), device-drawn noise, one SVGD step per period, no warm-up, B in {1, 4, 16, 64, 256}, every
plant with its own true (length, mass).  Four legs, in the same process on the same library build, alternating, REPS times each after a
warm-up:
  (off)    the call with recording off: svmpc_dual_sim_period_kernel;
  (theta)  ... recording the particles: svmpc_dual_sim_hist_period_kernel copies [N][H][da] per period and environment, and
           dust_svmpc_batch_get_history(DUST_HIST_THETA) reads the block back once;
  (both)   ... and the filters' particles [Mp][P], read back as well;
  (loop)   the loop a history had to drop back to before: per period one dust_svmpc_dual_batch_tick, dust_svmpc_batch_get(DUST_SVB_THETA)
           and dust_mpf_batch_get_particles, the B plants stepped on the host by one vectorised numpy step, the cost summed on the host.
A leg's time is a host clock around whole episodes, the read-back of the history included (each ends in a device synchronise).  T = 1 is
the control: an episode of one period has nothing to save.  Printed: the median environment-periods/s of each leg with its spread (min ..
max over the repeats) and the ratios off / theta, off / both (the cost of recording) and both / loop of the medians.
    python tools/svmpc_history_time.py [seconds per window, default 1.0] [largest B, default 256] [periods, default 64,1]"""
import math, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from dust_amd import Context, MpfContext, _lib as L

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
print("T B  leg env_periods_per_s [min max] us_per_period", flush=True)
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

        def cost(x):  # the demo's instantaneous cost
            return (np.float32(50.0) * (np.cos(x[:, 0]) - np.float32(1.0)) ** 2 + x[:, 1] ** 2).astype(np.float32)

        pairs = [pair(B, np.random.default_rng(B)) for _ in range(4)]
        for _, mb in pairs:
            mb.set_obs(states)
        pairs[1][0].set_history(theta=True)
        pairs[2][0].set_history(theta=True, filter=True)
        keys = (np.arange(B, dtype=np.uint64)[None] << np.uint64(32)) + np.arange(1, T + 1, dtype=np.uint64)[:, None]

        def sim(sb, mb):
            sb.dual_simulate(mb, states, T, 1, None, mpf_steps=MPF_STEPS, seeds=keys, plant_params=true, want_pw=False)

        def run_off(sb=pairs[0][0], mb=pairs[0][1]):
            sim(sb, mb)

        def run_theta(sb=pairs[1][0], mb=pairs[1][1]):
            sim(sb, mb)
            sb.history(L.HIST_THETA)

        def run_both(sb=pairs[2][0], mb=pairs[2][1]):
            sim(sb, mb)
            sb.history(L.HIST_THETA)
            sb.history(L.HIST_FILTER)

        def run_loop(sb=pairs[3][0], mb=pairs[3][1]):
            x, a, loss, th, xf = states, None, np.zeros(B, np.float32), [], []
            for t in range(T):
                a_seq, _, _, _ = sb.dual_tick(mb, x, a, n_steps=1, mpf_steps=MPF_STEPS, seeds=keys[t])
                th.append(sb.get(L.SVB_THETA))
                xf.append(mb.get_particles())
                a = a_seq[:, 0]
                x = step(x, a)
                loss = loss + cost(x)

        legs = (("off", run_off), ("theta", run_theta), ("theta+filter", run_both), ("loop", run_loop))
        n = [episodes_for(fn) for _, fn in legs]
        times = [[] for _ in legs]
        for _ in range(REPS):  # alternating: the legs see the same neighbours on the host and the device
            for k, (_, fn) in enumerate(legs):
                times[k].append(leg(fn, n[k]) / T)
        med = [float(np.median(t)) for t in times]
        for k, (name, _) in enumerate(legs):
            print("%3d %3d  %-13s %10.0f [%10.0f %10.0f]  %9.1f"
                  % (T, B, name, B / med[k], B / max(times[k]), B / min(times[k]), 1e6 * med[k]), flush=True)
        print("         off / theta %.3f   off / theta+filter %.3f   theta+filter / loop %.2f" % (med[1] / med[0], med[2] / med[0], med[3] / med[2]),
              flush=True)
        for sb, mb in pairs:
            sb.close()
            mb.close()
