"""A hyper-parameter sweep as one batch against what a tuning loop does without it.  Device-drawn noise, one SVGD step per period, episodes
of T periods at demo/pendulum_config.yaml's shape (Pendulum, N 3, S 128, M 8 (length, mass sampled), H 30), B distinct rows drawn from
demo/pendulum_tuning.py's search space (lr, alpha with temperature = 1 / alpha, prior_sigma), B in {1, 4, 16, 64, 256}:
  (s) ONE dust_svmpc_batch_episode of the batch WITH rows (svmpc_sweep_episode_kernel);
  (i) the same batch WITHOUT rows (svmpc_episode_kernel): what the per-environment loads and the mixed softmax paths cost;
  (ii) B one-environment batches, each a prototype of its own row, their episodes run in turn: what a tuning loop does today.
The three legs run in the same process, alternating, REPS times each after a warm-up; a leg's time is a host clock around whole episodes
(every episode call waits for the device and copies its records back).  T = 1 is the control: one period per launch, the launch and the
copy dominate.  Printed: the median environment-ticks/s of each leg with its spread (min .. max over the repeats).
    python tools/svmpc_sweep_time.py [seconds per window, default 1.0] [largest B, default 256] [periods per episode, default 64]"""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from dust_amd import Context

WINDOW = float(sys.argv[1]) if len(sys.argv) > 1 else 1.0
BMAX = int(sys.argv[2]) if len(sys.argv) > 2 else 256
T = int(sys.argv[3]) if len(sys.argv) > 3 else 64
REPS = 5
N, S, M, H = 3, 128, 8, 30
BASE = dict(model="pendulum", kernel="K1", N=N, S=S, M=M, H=H, uncertain_params=("length", "mass"), sigma_a=2.0)


def draw_rows(B, rng):
    lr = np.exp(rng.uniform(np.log(1e-1), np.log(1e2), B)).astype(np.float32).astype(np.float64)  # (a Context carries a plain lr in fp32)
    alpha = rng.uniform(1e-1, 1e1, B).astype(np.float32)
    sp = np.exp(rng.uniform(np.log(1e-1), np.log(1e2), B)).astype(np.float32)
    sa = np.full((B, 1), 2.0, np.float32)
    return dict(lr=lr, alpha=alpha, temperature=(1.0 / alpha).astype(np.float32), sigma_a=sa, chol_a=sa.copy(), sigma_p=sp.reshape(B, 1),
                weighted_prior=np.zeros(B, np.int64))


def proto_of(rows, b, th, mu):
    c = Context(seed=3, lr=float(rows["lr"][b]), alpha=float(rows["alpha"][b]), temperature=float(rows["temperature"][b]),
                sigma_p=float(rows["sigma_p"][b, 0]), **BASE)
    c.set_theta(th)
    c.set_prior(mu)
    c.set_a_mat(th)
    return c


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


print("T = %d periods per episode, %d repeats per leg; environment-ticks/s, median [min max]" % (T, REPS))
print("  B   one batch with rows              the same batch without rows      B one-environment batches in turn   rows/no-rows  rows/in-turn", flush=True)
for B in (1, 4, 16, 64, 256):
    if B > BMAX:
        continue
    rng = np.random.default_rng(S + B)
    rows = draw_rows(B, rng)
    mu = rng.standard_normal((N, H, 1)).astype(np.float32)
    th = (mu + 2 * rng.standard_normal((N, H, 1))).astype(np.float32)
    states = (np.array([3.0, 0.0], np.float32) + 0.1 * rng.standard_normal((B, 2))).astype(np.float32)
    params = np.ascontiguousarray(np.broadcast_to((1.0 + 0.1 * rng.standard_normal((1, B, 1, M, 2))).astype(np.float32), (T, B, 1, M, 2)))
    true = np.tile(rng.uniform(0.8, 1.2, (1, 2)).astype(np.float32), (B, 1))  # one plant for every trial, as the tuning script has it
    seeds = [3 + b for b in range(B)]
    p0 = proto_of(rows, 0, th, mu)
    swept, plain = p0.svmpc_batch(B, seeds=seeds), p0.svmpc_batch(B, seeds=seeds)
    p0.close()
    swept.set_hyper(rows)
    ones = []
    for b in range(B):
        p = proto_of(rows, b, th, mu)
        ones.append(p.svmpc_batch(1, seeds=seeds[b:b + 1]))
        p.close()
    params_one = [np.ascontiguousarray(params[:, b:b + 1]) for b in range(B)]

    def run_swept():
        swept.episode(states, T, 1, params, true, want_pw=False)

    def run_plain():
        plain.episode(states, T, 1, params, true, want_pw=False)

    def run_in_turn():
        for b in range(B):
            ones[b].episode(states[b:b + 1], T, 1, params_one[b], true[b:b + 1], want_pw=False)

    legs = (run_swept, run_plain, run_in_turn)
    n = [episodes_for(f) for f in legs]
    t = [[], [], []]
    for _ in range(REPS):  # alternating: the legs see the same neighbours on the host and the device
        for k, f in enumerate(legs):
            t[k].append(leg(f, n[k]) / T)
    med = [float(np.median(v)) for v in t]
    cols = "  ".join("%10.0f [%10.0f %10.0f]" % (B / med[k], B / max(t[k]), B / min(t[k])) for k in range(3))
    print("%3d  %s  %10.2f  %10.2f" % (B, cols, med[1] / med[0], med[2] / med[0]), flush=True)
    for b in [swept, plain] + ones:
        b.close()
