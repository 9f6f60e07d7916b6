"""dust_svmpc_batch_simulate against dust_svmpc_batch_episode in the same build.  Device-drawn noise, one SVGD step per period, T periods
per call, at demo/pendulum_config.yaml's shape - Pendulum, N 3, S 128, M 8 (length, mass sampled), H 30 -, B in {1, 4, 16, 64, 256}:
  (r) ONE dust_svmpc_batch_simulate with the rules off (warm_up 0, no goal, no crash rule): the episode plus the cost record, the fp32
      loss and the three per-environment words;
  (e) ONE dust_svmpc_batch_episode: its kernels are the text they were before the rules came, so this leg is the baseline;
  (w) ONE dust_svmpc_batch_simulate with warm_up = 30: the first 30 periods are optimize alone, with no forward().
The three legs run in the same process, alternating, REPS times each after a warm-up; a leg's time is a host clock around whole calls.
Printed: the median environment-periods/s of each leg with its spread (min .. max over the repeats), and r / e, w / e of the medians.
    python tools/svmpc_sim_time.py [seconds per window, default 1.0] [largest B, default 256] [periods per call, default 64]"""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from dust_amd import Context

WINDOW = float(sys.argv[1]) if len(sys.argv) > 1 else 1.0
BMAX = int(sys.argv[2]) if len(sys.argv) > 2 else 256
T = int(sys.argv[3]) if len(sys.argv) > 3 else 64
REPS, WARM_UP = 5, 30
N, S, M, H = 3, 128, 8, 30


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


print("T = %d periods per call, %d repeats per leg, warm_up = %d in leg w" % (T, REPS, WARM_UP))
print("  B  rules_off_env_periods_per_s [min max]  episode_env_periods_per_s [min max]  warm_up_env_periods_per_s [min max]  r/e  w/e", flush=True)
for B in (1, 4, 16, 64, 256):
    if B > BMAX:
        continue
    rng = np.random.default_rng(S + B)
    states = (np.array([3.0, 0.0], np.float32) + 0.1 * rng.standard_normal((B, 2))).astype(np.float32)
    params = np.ascontiguousarray(np.broadcast_to((1.0 + 0.1 * rng.standard_normal((B, 1, M, 2))).astype(np.float32)[None], (T, B, 1, M, 2)))
    true = rng.uniform(0.8, 1.2, (B, 2)).astype(np.float32)
    mu = rng.standard_normal((N, H, 1)).astype(np.float32)
    th = (mu + 2 * rng.standard_normal((N, H, 1))).astype(np.float32)
    proto = Context(seed=3, model="pendulum", kernel="K1", lr=2.0, sigma_a=2.0, sigma_p=2.0, N=N, S=S, M=M, H=H, uncertain_params=("length", "mass"))
    proto.set_theta(th)
    proto.set_prior(mu)
    proto.set_a_mat(th)
    batches = [proto.svmpc_batch(B, seeds=[3 + b for b in range(B)]) for _ in range(3)]
    proto.close()
    legs = [lambda b=batches[0]: b.simulate(states, T, 1, params, true, want_pw=False),
            lambda b=batches[1]: b.episode(states, T, 1, params, true, want_pw=False),
            lambda b=batches[2]: b.simulate(states, T, 1, params, true, warm_up=WARM_UP, want_pw=False)]
    n = [calls_for(fn) for fn in legs]
    t = [[], [], []]
    for _ in range(REPS):  # alternating: the legs see the same neighbours on the host and the device
        for k, fn in enumerate(legs):
            t[k].append(leg(fn, n[k]) / T)
    med = [float(np.median(v)) for v in t]
    print("%3d  " % B + "  ".join("%10.0f [%10.0f %10.0f]" % (B / med[k], B / max(t[k]), B / min(t[k])) for k in range(3))
          + "  %5.3f  %5.3f" % (med[1] / med[0], med[1] / med[2]), flush=True)
    for b in batches:
        b.close()
