"""AMPPI episodes under the reference's rules on the device (dust_amppi_batch_simulate, dust_amppi_dual_batch_simulate) against what they
replace.  Pendulum, H 30, S 1 024, "extended" rows over (length, mass), device-drawn noise, B in {1, 4, 16, 64, 256}, every plant with
its own true (length, mass); the dual pair with 256 filter particles, 20 filter steps per update, Silverman's bandwidth.  Four legs per
pair, in the same process on the same library build, alternating, REPS times each after a warm-up:
  (s0) ONE simulate call of T periods with the rules off (no goal, no crash rule);
  (e)  ONE plain episode call of T periods: what (s0) computes, bit for bit - the cost of the rules' bookkeeping is (s0) / (e);
  (sg) ONE simulate call of T periods with a goal rule (out of reach: every environment runs all T periods);
  (l)  the loop (sg) replaces, T times: dust_amppi_batch_update with a_seq read back (dual: dust_amppi_dual_batch_tick), the B plants
       stepped on the host by one vectorised numpy step, the cost and the goal predicate on the host, dust_amppi_batch_roll.
A leg's time is a host clock around whole episodes (each ends in a device synchronise).  T = 1 is the control: an episode of one period
has nothing to save.  Printed: the median environment-periods/s of each leg with its spread (min .. max over the repeats), the ratios
(s0) / (e) and (sg) / (l) of the medians, and whether the rules-off leg lies inside the repeats' spread of the plain episode.
    python tools/amppi_sim_time.py [seconds per window, default 1.0] [largest B, default 256] [periods, default 64,1] [plain,dual]"""
import math, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from dust_amd import Context, MpfContext

WINDOW = float(sys.argv[1]) if len(sys.argv) > 1 else 1.0
BMAX = int(sys.argv[2]) if len(sys.argv) > 2 else 256
PERIODS = [int(v) for v in (sys.argv[3] if len(sys.argv) > 3 else "64,1").split(",")]
KINDS = (sys.argv[4] if len(sys.argv) > 4 else "plain,dual").split(",")
REPS = 5
S, H, MP, MPF_STEPS = 1024, 30, 256, 20
GOAL, RADIUS = (0.0, 0.0), 1e-3


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


def pair(B, rng, dual):
    """a controller batch (and, dual, a filter batch) of B environments"""
    proto = Context(model="pendulum", N=1, S=S, M=1, H=H, temperature=100.0, alpha=0.01, sigma_a=2.0, uncertain_params=("length", "mass"), seed=3)
    ab = proto.amppi_batch(B, seeds=[3 + b for b in range(B)])
    proto.close()
    if not dual:
        return ab, None
    x0 = (1.0 + 0.1 * rng.standard_normal((B, MP, 2))).astype(np.float32)
    m = MpfContext(x0[0], np.array([3.0, 0.0], np.float32), model="pendulum", uncertain_params=("length", "mass"), obs_std=0.1, lr=1e-3, init_bw=0.1)
    mb = m.batch(B)
    m.close()
    mb.set_particles(x0)
    return ab, mb


print("%d repeats per leg, windows of %.1f s" % (REPS, WINDOW))
print("kind T B  leg env_periods_per_s [min max] us_per_period", flush=True)
for kind in KINDS:
    dual = kind == "dual"
    for T in PERIODS:
        for B in (1, 4, 16, 64, 256):
            if B > BMAX:
                continue
            rng = np.random.default_rng(S + B)
            states = (np.array([3.0, 0.0], np.float32) + 0.1 * rng.standard_normal((B, 2))).astype(np.float32)
            true = rng.uniform(0.8, 1.2, (B, 2)).astype(np.float32)
            c0, c1 = (-3.0 * 9.8 / (2.0 * true[:, 0])).astype(np.float32), (3.0 / (true[:, 1] * true[:, 0] ** 2)).astype(np.float32)
            params = None if dual else (1.0 + 0.1 * rng.standard_normal((T, B, S, 2))).astype(np.float32)
            goal, r2 = np.asarray(GOAL, np.float32), np.float32(RADIUS * RADIUS)

            def step(x, a):  # pendulum.py:82-100 for B plants at once
                u = np.clip(a[:, 0], -2.0, 2.0)
                thd = np.clip(x[:, 1] + np.float32(0.05) * (c0 * np.sin(x[:, 0] + np.float32(math.pi)) + c1 * u), -8.0, 8.0)
                return np.stack((x[:, 0] + thd * np.float32(0.05), thd), 1).astype(np.float32)

            def cost(x):  # the demo's instantaneous cost
                return (np.float32(50.0) * (np.cos(x[:, 0]) - np.float32(1.0)) ** 2 + x[:, 1] ** 2).astype(np.float32)

            pairs = [pair(B, np.random.default_rng(B), dual) for _ in range(4)]
            for _, mb in pairs:
                if mb is not None:
                    mb.set_obs(states)
            keys = (np.arange(B, dtype=np.uint64)[None] << np.uint64(32)) + np.arange(1, T + 1, dtype=np.uint64)[:, None]

            def sim(ab, mb, **rules):
                if dual:
                    ab.dual_simulate(mb, states, T, None, mpf_steps=MPF_STEPS, seeds=keys, plant_params=true, want_costs=False, **rules)
                else:
                    ab.simulate(states, T, params, plant_params=true, want_costs=False, **rules)

            def run_sim0(ab=pairs[0][0], mb=pairs[0][1]):
                sim(ab, mb)

            def run_episode(ab=pairs[1][0], mb=pairs[1][1]):
                if dual:
                    ab.dual_episode(mb, states, T, None, mpf_steps=MPF_STEPS, seeds=keys, plant_params=true, want_costs=False)
                else:
                    ab.episode(states, T, params, plant_params=true, want_costs=False)

            def run_simg(ab=pairs[2][0], mb=pairs[2][1]):
                sim(ab, mb, goal=GOAL, goal_radius=RADIUS)

            def run_loop(ab=pairs[3][0], mb=pairs[3][1]):
                x, a, loss, on = states, None, np.zeros(B, np.float32), np.ones(B, np.uint8)
                for t in range(T):
                    if dual:
                        _, _, a_seq, _, _ = ab.dual_tick(mb, x, a, None, mpf_steps=MPF_STEPS, seeds=keys[t], roll=1, active=on)
                    else:
                        _, _, a_seq, _ = ab.update(x, None, params[t], active=on, want_costs=False)
                        ab.roll(1, active=on)
                    a = np.nan_to_num(a_seq[:, 0])
                    x = np.where(on[:, None] != 0, step(x, a), x)
                    loss = loss + np.where(on != 0, cost(x), np.float32(0.0))
                    d = goal - x
                    on = on & ~((d * d).sum(1) <= r2)
                    if not on.any():
                        break

            legs = (("sim_rules_off", run_sim0), ("episode", run_episode), ("sim_goal", run_simg), ("loop", run_loop))
            n = [episodes_for(fn) for _, fn in legs]
            times = [[] for _ in legs]
            for _ in range(REPS):  # alternating: the legs see the same neighbours on the host and the device
                for k, (_, fn) in enumerate(legs):
                    times[k].append(leg(fn, n[k]) / T)
            med = [float(np.median(t)) for t in times]
            for k, (name, _) in enumerate(legs):
                print("%-5s %3d %3d  %-13s %10.0f [%10.0f %10.0f]  %9.1f"
                      % (kind, T, B, name, B / med[k], B / max(times[k]), B / min(times[k]), 1e6 * med[k]), flush=True)
            inside = min(times[1]) <= med[0] <= max(times[1])
            print("               sim_rules_off / episode %.3f (the rules-off median lies %s the plain episode's spread)   sim_goal / loop %.2f"
                  % (med[1] / med[0], "inside" if inside else "OUTSIDE", med[3] / med[2]), flush=True)
            for ab, mb in pairs:
                ab.close()
                if mb is not None:
                    mb.close()
