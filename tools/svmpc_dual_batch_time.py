"""Closed-loop environment-periods per second of the DuSt-MPC loop over B plants, three legs in the same process on the same device:
  (a) ONE BatchDualSVMPC of B environments: a period of all of them is one C call (dust_svmpc_dual_batch_tick) - the filters' launches
      and the tick's launch on one stream, the dynamics samples drawn inside the tick's kernel;
  (b) the composition by hand of the batched pieces: MpfBatch.optimize (ends in a stream synchronisation), the B x Mp x P particles and
      the bandwidths read back, B draws of [n_steps, M, P] with torch on the host (one per environment, as BatchSVMPC._params makes them),
      BatchSVMPC.tick, which uploads the rows;
  (c) B lone DualSVMPC(fused=True) objects stepped one after the other: B C calls per period, each with its own filter launches, its
      4-byte bandwidth round trip and its synchronisations.
Scenario: examples/svmpc_dual_batch_example.py - Pendulum (length, mass) at the demo's SVMPC shape (N 3, S 128, M 8, H 30, one SVGD step
per period), 256 filter particles, 20 filter steps, Silverman bandwidths, numpy pendulums with their own true parameters as plants - at
B in {1, 4, 16, 64, 256}.  A period ends with every environment's action on the host (the plants need it), so every timed window ends
synchronised.  All legs are warmed up (contexts, code objects, the first filter update), then timed REPS times each, alternating;
printed: the median environment-periods/s of each leg with its spread (min .. max over the repeats) and the ratios (b) / (a) and
(c) / (a) of the median period times (> 1: the batch class is faster).

    python tools/svmpc_dual_batch_time.py [seconds per window, default 1.0] [largest B, default 256]"""
import importlib.util
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

WINDOW = float(sys.argv[1]) if len(sys.argv) > 1 else 1.0
BMAX = int(sys.argv[2]) if len(sys.argv) > 2 else 256
REPS, WARM = 5, 5
KW = dict(particles=3, samples=128, params=8, horizon=30, mpf_particles=256, seed=0, mpf_bw=None, mpf_steps=20)


def example():
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples", "svmpc_dual_batch_example.py")
    spec = importlib.util.spec_from_file_location("svmpc_dual_batch_example", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def pendulum(states, actions, length, mass, dt=0.05, g=9.8, max_torque=2.0, max_speed=8.0):
    """the plants: rows of (theta, theta_dot) under each row's own length and mass, vectorised over the rows"""
    x, u = np.asarray(states, np.float32).reshape(-1, 2), np.clip(np.asarray(actions, np.float32).reshape(-1), -max_torque, max_torque)
    thd = x[:, 1] + dt * (-3.0 * g / (2.0 * length) * np.sin(x[:, 0] + np.pi) + 3.0 / (mass * length ** 2) * u)
    thd = np.clip(thd, -max_speed, max_speed)
    return torch.from_numpy(np.stack([x[:, 0] + thd * dt, thd], 1).astype(np.float32))


class ByHand:
    """leg (b): the loop of BatchDualSVMPC out of the calls that exist without it"""

    def __init__(self, loop):
        self.loop, self.prev = loop, None
        self.gen = torch.Generator().manual_seed(1)

    def period(self, states, plant):
        loop = self.loop
        sv, B = loop.svmpc, loop.n_envs
        st = sv._states(states)
        mb = loop._filters(st)
        if self.prev is not None:
            mb.optimize(self.prev, st, loop.mpf_bw, loop.mpf_steps)  # (synchronises)
        x, bw = torch.from_numpy(mb.get_particles()), torch.from_numpy(mb.get_prior_bw())  # [B, Mp, P], [B, P]
        n_steps, M = sv.n_steps, sv.likelihood.controller.n_params
        rows = []
        for b in range(B):  # one draw per environment from ITS prior: a uniform mixture of N(x_j, diag(bw^2))
            k = torch.randint(x.shape[1], (n_steps, M), generator=self.gen)
            rows.append(x[b][k] + bw[b] * torch.randn(n_steps, M, x.shape[2], generator=self.gen))
        a_seq, _ = sv.tick(states, loop.mpf.prior, params=torch.stack(rows))
        actions = a_seq[:, 0]
        new = plant(states, actions)
        self.prev = actions.numpy().copy()
        return new


def lone(ex, b, n_envs, particles, samples, params, horizon, mpf_particles, seed, mpf_bw, mpf_steps):
    """environment b of the example's scenario as a DualSVMPC(fused=True) of its own"""
    from dust_amd.controllers import DualSVMPC, MultiDISCO
    from dust_amd.costs import PendulumQuadCos
    from dust_amd.inference import MPF, SVMPC, ExponentiatedUtility, GaussianLikelihood, get_gmm
    from dust_amd.kernels import RBFKernel
    from dust_amd.models import PendulumModel

    _, _, start = ex.truths(n_envs, seed)
    g = torch.Generator().manual_seed(2000 + seed)
    x0 = 1.0 + 0.1 * torch.randn(n_envs, mpf_particles, 2, generator=g)
    model, cost = PendulumModel(uncertain_params=("length", "mass")), PendulumQuadCos()
    ctrl = MultiDISCO(model.observation_space, model.action_space, horizon, particles, samples, temperature=1.0, a_cov=ex.A_COV * torch.eye(1),
                      inst_cost_fn=cost.inst_cost, term_cost_fn=cost.term_cost, params_sampling=True, params_samples=params, seed=seed + b)
    ctrl.return_rollouts = False
    prior = get_gmm(torch.zeros(particles, horizon, 1), torch.ones(particles), ex.A_COV * torch.eye(1))
    init = ex.A_COV ** 0.5 * torch.randn(n_envs, particles, horizon, 1, generator=g)
    sv = SVMPC(likelihood=ExponentiatedUtility(alpha=1.0, n_samples=samples, controller=ctrl, model=model), init_particles=init[b], prior=prior,
               kernel=RBFKernel(), n_particles=particles, n_steps=1, optimizer_class=torch.optim.SGD, lr=1.0)
    mpf = MPF(init_particles=x0[b], likelihood=GaussianLikelihood(initial_obs=start[b], obs_std=ex.OBS_STD, model=model, log_space=False),
              optimizer_class=torch.optim.SGD, lr=ex.LR, bw=ex.INIT_BW, bw_scale=1.0)
    return DualSVMPC(sv, mpf, mpf_bw=mpf_bw, mpf_steps=mpf_steps, fused=True, seed=seed + (b << 32))


def window(period, state, n):
    t0 = time.perf_counter()
    for _ in range(n):
        state = period(state)  # (the actions came to the host inside: the streams are drained)
    return (time.perf_counter() - t0) / n, state


def main():
    ex = example()
    print("B  (a) batch_class env_periods_per_s [min max]  (b) by_hand [min max]  (c) lone_objects [min max]  us_per_period a b c  b/a c/a", flush=True)
    for B in (1, 4, 16, 64, 256):
        if B > BMAX:
            break
        loop, _, start, (length, mass) = ex.scenario(n_envs=B, **KW)
        hand = ByHand(ex.scenario(n_envs=B, **KW)[0])
        lones = [lone(ex, b, B, **KW) for b in range(B)]
        length, mass = length.numpy().astype(np.float64), mass.numpy().astype(np.float64)
        plant = lambda x, u: pendulum(x, u, length, mass)
        plants = [lambda x, u, b=b: pendulum(x, u, length[b:b + 1], mass[b:b + 1]) for b in range(B)]
        legs = [lambda s: loop.tick(s, plant)[1], lambda s: hand.period(s, plant),
                lambda ss: [lo.tick(s, pl)[1] for lo, pl, s in zip(lones, plants, ss)]]
        states = [start.clone(), start.clone(), [start[b].reshape(1, -1) for b in range(B)]]
        n = []
        for k, leg in enumerate(legs):
            _, states[k] = window(leg, states[k], WARM)
            p, states[k] = window(leg, states[k], 3)
            n.append(max(3, int(WINDOW / p)))
        times = [[], [], []]
        for _ in range(REPS):  # alternating: the legs see the same neighbours on the host and the device
            for k, leg in enumerate(legs):
                t, states[k] = window(leg, states[k], n[k])
                times[k].append(t)
        ok = bool(torch.isfinite(states[0]).all()) and bool(torch.isfinite(states[1]).all()) and all(bool(torch.isfinite(s).all()) for s in states[2])
        med = [float(np.median(t)) for t in times]
        print("%3d  " % B + "  ".join("%9.0f [%9.0f %9.0f]" % (B / m, B / max(t), B / min(t)) for m, t in zip(med, times)) +
              "  %10.1f %10.1f %10.1f  %6.2f %6.2f%s" % (1e6 * med[0], 1e6 * med[1], 1e6 * med[2], med[1] / med[0], med[2] / med[0],
                                                        "" if ok else "  NON-FINITE STATE"), flush=True)
        for lp in (loop, hand.loop):
            lp.svmpc._batch.close()
            lp._mb.close()
        for lo in lones:
            lo.controller._ctx.close()
            lo.mpf._dev.close()


if __name__ == "__main__":
    main()
