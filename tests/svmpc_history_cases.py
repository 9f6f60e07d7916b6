"""Cases (TEST INFRASTRUCTURE) for the posterior's history - dust_svmpc_batch_set_history / dust_svmpc_batch_get_history, the recording
kernels svmpc_sim_hist_kernel and svmpc_dual_sim_hist_period_kernel -, shared by tests/test_svmpc_history_cpu.py and
tests/test_gpu_svmpc_history.py.  Data only: nothing here imports the library.

The cases are built by the constructors of tests/svmpc_dual_sim_cases.py (a dual-episode case plus rules) and tests/svmpc_sim_cases.py
(an episode case plus rules), so that start states, particles, true rows, seeds and the fp32 rule replicas are imported and never
restated.  The shapes are the smallest at which a history row can still go wrong:

  P1  Pendulum, SGD / K1, N 3, S 8, M 2, H 4, B 3, T 5, warm_up 2; Mp 3, P 2, Silverman: warm-up rows (the optimiser's step closes the
      period, not the roll), an update-free period 0 (the filter row is the particles at entry); theta row 12 floats (quads), filter row 6
  P2  Pendulum, Adam / IMQ, n_steps 3, N 4, S 8, M 3, H 5, T 4, warm_up 1; Mp 65, log space, called WITH actions_prev: row 0 lies behind
      an update; a filter row (130 floats, no quads) wider than one wave
  P3  Particle on its map, roll "mean", weighted prior, T 4; Mp 130, P 1; the forced crash / goal starts of svmpc_dual_sim_cases
      `part_events`: rows at or past n_run stay unwritten; a ragged filter row
  P4  N = S = M = H = T = Mp = P = 1: every bound
  P5  skid-steer and cart-pole, plain simulate, N 8, S 8, M 2, H 6, T 4: the two families the dual call does not take
  P6  Particle, plain simulate, N 64, H 64 (D = 128), S 4, M 1, T 2: the widest theta row (8192 floats: 2048 quads, four strides of the
      512 lanes)
and one beyond the issue's list, for the two copy paths the six leave out:
  P7  Pendulum, N 3, H 5 (theta row 15 floats: the scalar path with more than one element), Mp 64, P 2 (filter row 128 floats: quads)
"""
import svmpc_dual_sim_cases as dsc
import svmpc_sim_cases as sc

_SGD = dict(kernel="K1", optimizer="SGD", lr=2.0, sigma_p=2.0)
_ADAM = dict(kernel="IMQ", optimizer="Adam", lr=0.5, sigma_p=2.0)
_PART = dict(kernel="K1", optimizer="SGD", lr=100.0, sigma_p=5.0, roll_strategy="mean", weighted_prior=True)
_PART_START = dsc.BY_ID["part_events"]["start"]  # 0 starts on an occupied cell, 1 inside the goal radius, 2 and 3 run on

# the dual cases (dust_svmpc_dual_batch_simulate); P1, P3, P4 and P7 also run the plain call on the same prototype
DUAL = [
    dsc._case("P1", "pendulum", 3, 8, 2, 4, 1, 5, 3, ("length", "mass"), 4101, _SGD, 1.0, ((1.25, 0.8), (0.8, 1.2), (1.15, 1.3)), 3, 2, None, "SGD",
              start=dsc.dec.PEND_START, rules=dict(warm_up=2)),
    dsc._case("P2", "pendulum", 4, 8, 3, 5, 3, 4, 2, ("length", "mass"), 4102, _ADAM, 1.0, ((0.85, 1.3), (1.2, 0.7)), 65, 2, 0.3, "Adam", log=True,
              first=True, start=dsc.dec.PEND_START, rules=dict(warm_up=1)),
    dsc._case("P3", "particle", 3, 8, 4, 4, 1, 4, 4, ("mass",), 4103, _PART, 3.0, ((1.3,), (0.75,), (0.85,), (1.15,)), 130, 2, 0.5, "SGD",
              start=_PART_START, rules=dict(goal=dsc.PART_GOAL, radius=1.0, crash=True)),
    dsc._case("P4", "pendulum", 1, 1, 1, 1, 1, 1, 1, ("length",), 4104, _SGD, 1.0, ((1.3,),), 1, 1, 0.1, "SGD", start=dsc.dec.PEND_START),
    dsc._case("P7", "pendulum", 3, 8, 2, 5, 1, 3, 2, ("length", "mass"), 4107, _SGD, 1.0, ((1.25, 0.8), (0.8, 1.2)), 64, 2, None, "SGD",
              start=dsc.dec.PEND_START, rules=dict(warm_up=1)),
]
for _c in DUAL:
    _c["rows"] = False  # (the key the plain call's helpers read: no per-environment controller rows)
DUAL_BY_ID = {c["id"]: c for c in DUAL}
DUAL_IDS = [c["id"] for c in DUAL]
# what P3's starts force, whatever the controller picks (proved for these starts by svmpc_dual_sim_cases.forced_events on `part_events`)
DUAL_EVENTS = {"P3": {0: (0, 2), 1: (0, 1)}}

# the plain cases (dust_svmpc_batch_simulate)
PLAIN = [
    sc._case("P5_skid", "skid", 8, 8, 2, 6, 1, 4, 2, ("x_icr",), 4105, dict(kernel="IMQ", optimizer="SGD", lr=0.05, sigma_p=0.3), 0.3, dict(warm_up=1),
             true_rel=((1.5,), (0.6,))),
    sc._case("P5_cart", "cartpole", 8, 8, 2, 6, 1, 4, 2, ("mass_pole", "length"), 4115, dict(kernel="K1", optimizer="SGD", lr=0.05, sigma_p=0.5), 0.5,
             dict(warm_up=1), true_rel=((2.0, 0.6), (0.5, 1.5))),
    sc._case("P6", "particle", 64, 4, 1, 64, 1, 2, 2, (), 4106, dict(kernel="K1", optimizer="SGD", lr=1.0, sigma_p=5.0), 3.0, dict(),
             start=((4.4, 0.3, -3.0, 4.5), (6.03, -8.04, -2.0, 1.0))),
]
# P1, P4, P7 (Pendulum) and P3 (Particle, with its stops) on the plain call: the controller side of the dual case; P2 is a dual case only
# (its point is the update behind actions_prev), and its log-space rows mean nothing to the plain call's parameter samples
PLAIN_FROM_DUAL = ["P1", "P3", "P4", "P7"]
PLAIN_BY_ID = dict({c["id"]: c for c in PLAIN}, **{k: DUAL_BY_ID[k] for k in PLAIN_FROM_DUAL})
PLAIN_IDS = PLAIN_FROM_DUAL + [c["id"] for c in PLAIN]

# the size cap's case: N 64, D 128, T 4096, B 9 - 9 x 2^25 values, more than 2^28; nothing of that size is ever allocated
CAP = dict(N=64, H=64, T=4096, B=9)

# the six recording instances, by the names the compiler gives them
MODELS = dict(pendulum=0, particle=1, skid=2, cartpole=3)
HIST_KERNELS = (["_ZN4dust21svmpc_sim_hist_kernelILi%dEEEvNS_16SvmpcSimHistArgsE" % m for m in range(4)] +
                ["_ZN4dust33svmpc_dual_sim_hist_period_kernelILi%dEEEvNS_26SvmpcDualSimHistPeriodArgsE" % m for m in range(2)])
