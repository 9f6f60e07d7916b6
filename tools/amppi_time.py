"""One AMPPI tick against what served "MPPI" before it: Pendulum, H = 30, S in {1024, 8192}, params_sampling="extended", device noise.
  (a) dust_amppi_update through the Context, nothing read back: open-loop ticks/s (enqueue-bound or kernel-bound, whichever is slower)
      and the kernel's own time from the profile counters (one HIP-event pair per launch);
  (b) the same through the AMPPI class (host parameter draws, costs and omega copied back);
  (c) MultiDISCO(n_policies=1, action_samples=S, params_samples=4) forward + step("average") - a different algorithm (M x S cross
      product, costs on t = 0 .. H - 1, two launches and more) - with its launches counted by the same counters.
    python tools/amppi_time.py [ticks]"""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
import torch.distributions as dist
from dust_amd import Context
from dust_amd.controllers import AMPPI, MultiDISCO
from dust_amd.costs import PendulumQuadCos
from dust_amd.models import PendulumModel

T = int(sys.argv[1]) if len(sys.argv) > 1 else 300
H, LAM, SIGMA = 30, 100.0, 2.0
state = np.array([3.0, 0.0], np.float32)
cost = PendulumQuadCos()


def timed(fn, sync, n=T, warm=20):
    for _ in range(warm):
        fn()
    sync()
    t0 = time.perf_counter()
    for _ in range(n):
        fn()
    sync()
    return (time.perf_counter() - t0) / n


for S in (1024, 8192):
    rng = np.random.default_rng(S)
    rows = (1.0 + 0.1 * rng.standard_normal((S, 1))).astype(np.float32)
    c = Context(model="pendulum", N=1, S=S, M=1, H=H, temperature=LAM, alpha=1.0 / LAM, sigma_a=SIGMA, uncertain_params=("length",), sampling=True, seed=3)
    c.set_a_seq((0.5 * rng.standard_normal((H, 1))).astype(np.float32))
    tick = timed(lambda: c.amppi_update(state, None, rows, want_outputs=False), c.sync)
    c.profile(True)
    for _ in range(50):
        c.amppi_update(state, None, rows, want_outputs=False)
    prof = c.profile_get()
    c.profile(False)
    (ms, n), = prof.values()
    print("S %5d  AMPPI Context, no read-back : %7.1f us per tick (%6.0f ticks/s); kernel %6.1f us; launches per tick: %s"
          % (S, 1e6 * tick, 1.0 / tick, 1e3 * ms / n, {k: v[1] / 50 for k, v in prof.items()}), flush=True)
    c.close()

    model = PendulumModel(uncertain_params=("length",))
    model.params_dist = dist.MultivariateNormal(torch.tensor([1.0]), covariance_matrix=0.01 * torch.eye(1))
    a = AMPPI(model.observation_space, model.action_space, H, S, lambda_=LAM, a_cov=SIGMA ** 2 * torch.eye(1), inst_cost_fn=cost.inst_cost,
              term_cost_fn=cost.term_cost, params_sampling="extended", seed=3)
    a.return_rollouts = False
    st = torch.tensor(state)
    tick = timed(lambda: a.update_actions(model, st), lambda: None)
    print("S %5d  AMPPI class (host draws, costs + omega back): %7.1f us per tick (%6.0f ticks/s)" % (S, 1e6 * tick, 1.0 / tick), flush=True)

    d = MultiDISCO(model.observation_space, model.action_space, H, 1, S, temperature=LAM, a_cov=SIGMA ** 2 * torch.eye(1), inst_cost_fn=cost.inst_cost,
                   term_cost_fn=cost.term_cost, params_sampling=True, params_samples=4, seed=3)
    d.return_rollouts = False

    def disco():
        d.forward(st, model, model.params_dist)
        d.step("average")

    tick = timed(disco, lambda: None)
    d._ctx.profile(True)
    for _ in range(50):
        disco()
    prof = d._ctx.profile_get()
    d._ctx.profile(False)
    print("S %5d  MultiDISCO(n_policies=1) forward + step('average'): %7.1f us per tick (%6.0f ticks/s); kernels %6.1f us; launches per tick: %s"
          % (S, 1e6 * tick, 1.0 / tick, 1e3 * sum(v[0] for v in prof.values()) / 50, {k: v[1] / 50 for k, v in prof.items()}), flush=True)
