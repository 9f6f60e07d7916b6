#!/usr/bin/env python3
"""B episodes of the DuSt-MPC loop at once on the MI355X backend: `BatchDualSVMPC` runs B pendulums, each with its OWN true mass and
length, on one `BatchSVMPC` (the control side: B ticks in one launch, at the shape of the reference's pendulum demo - 3 Stein particles,
128 action samples, 8 dynamics samples, horizon 30, one SVGD step per period) and B copies of one `MPF` (the dynamics side: B filter
updates in one launch) - the batch counterpart of `DualSVMPC(fused=True)`, and the sibling of examples/amppi_dual_batch_example.py and
examples/svmpc_batch_example.py.  The reference evaluates the dual controller over many episodes and gives each a deep copy of the
controller and of the filter (dust/utils/simulations.py:62,78); here a control period of all of them is one C call
(dust_svmpc_dual_batch_tick) whose number of kernel launches does not depend on B: every workgroup of the tick's kernel draws its
environment's dynamics samples from that environment's refreshed filter prior.  The plants are host `PendulumModel`s.

    python examples/svmpc_dual_batch_example.py --envs 8 --ticks 100
"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from dust_amd.controllers import BatchDualSVMPC, MultiDISCO  # noqa: E402
from dust_amd.costs import PendulumQuadCos  # noqa: E402
from dust_amd.inference import MPF, BatchSVMPC, ExponentiatedUtility, GaussianLikelihood, get_gmm  # noqa: E402
from dust_amd.kernels import RBFKernel  # noqa: E402
from dust_amd.models import PendulumModel  # noqa: E402

A_COV, LR, OBS_STD, INIT_BW = 4.0, 1e-3, 0.1, 0.1


def truths(n_envs, seed=0):
    """-> (true lengths [B], true masses [B], start states [B, 2])"""
    g = torch.Generator().manual_seed(1000 + seed)
    length = 0.8 + 0.5 * torch.rand(n_envs, generator=g)
    mass = 0.8 + 0.5 * torch.rand(n_envs, generator=g)
    start = torch.tensor([3.0, 0.0]) + 0.2 * torch.randn(n_envs, 2, generator=g)
    return length, mass, start


def scenario(n_envs=8, particles=3, samples=128, params=8, horizon=30, mpf_particles=256, seed=0, mpf_bw=None, mpf_steps=20, n_steps=1):
    """-> (loop, plant(states [B, 2], actions [B, 1]) -> new states, start states [B, 2], (true lengths, true masses))"""
    length, mass, start = truths(n_envs, seed)
    g = torch.Generator().manual_seed(2000 + seed)
    x0 = 1.0 + 0.1 * torch.randn(n_envs, mpf_particles, 2, generator=g)  # every environment's belief over (length, mass), round (1, 1)
    model, cost = PendulumModel(uncertain_params=("length", "mass")), PendulumQuadCos()
    ctrl = MultiDISCO(model.observation_space, model.action_space, horizon, particles, samples, temperature=1.0, a_cov=A_COV * torch.eye(1),
                      inst_cost_fn=cost.inst_cost, term_cost_fn=cost.term_cost, params_sampling=True, params_samples=params, seed=seed)
    prior = get_gmm(torch.zeros(particles, horizon, 1), torch.ones(particles), A_COV * torch.eye(1))
    init = A_COV ** 0.5 * torch.randn(n_envs, particles, horizon, 1, generator=g)  # every episode starts from its own particles
    lik = ExponentiatedUtility(alpha=1.0, n_samples=samples, controller=ctrl, model=model)
    svmpc = BatchSVMPC(n_envs, init, prior, lik, kernel=RBFKernel(), n_particles=particles, n_steps=n_steps, optimizer_class=torch.optim.SGD,
                       lr=1.0, seeds=[seed + b for b in range(n_envs)])
    mpf = MPF(init_particles=x0[0], likelihood=GaussianLikelihood(initial_obs=start[0], obs_std=OBS_STD, model=model, log_space=False),
              optimizer_class=torch.optim.SGD, lr=LR, bw=INIT_BW, bw_scale=1.0)
    loop = BatchDualSVMPC(svmpc, mpf, mpf_bw=mpf_bw, mpf_steps=mpf_steps, seed=seed, init_particles=x0)
    plants = [PendulumModel(length=float(length[b]), mass=float(mass[b])) for b in range(n_envs)]

    def plant(states, actions):
        states, actions = torch.as_tensor(states, dtype=torch.float), torch.as_tensor(actions, dtype=torch.float)
        return torch.stack([plants[b].step(states[b].reshape(1, -1), actions[b].reshape(1, -1)).reshape(-1) for b in range(n_envs)])

    return loop, plant, start, (length, mass)


def main(argv=None):
    """-> the plants' states [ticks + 1, B, 2]"""
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=8)
    ap.add_argument("--ticks", type=int, default=100)
    ap.add_argument("--particles", type=int, default=3)
    ap.add_argument("--samples", type=int, default=128)
    ap.add_argument("--params", type=int, default=8)
    ap.add_argument("--horizon", type=int, default=30)
    ap.add_argument("--mpf-particles", type=int, default=256)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--verbose", action="store_true")
    a = ap.parse_args(argv)
    loop, plant, start, (length, mass) = scenario(a.envs, a.particles, a.samples, a.params, a.horizon, a.mpf_particles, a.seed)
    states, trace = start.clone(), [start.clone()]
    for t in range(a.ticks):
        actions, states, _ = loop.tick(states, plant)
        trace.append(states.clone())
        if a.verbose:
            print("tick %3d  torque %s" % (t, " ".join("%+.2f" % float(u) for u in actions.reshape(-1))))
    x = loop.dyn_particles.mean(1)
    err0 = float(((1.0 - length) ** 2 + (1.0 - mass) ** 2).sqrt().mean())
    err1 = float(((x[:, 0] - length) ** 2 + (x[:, 1] - mass) ** 2).sqrt().mean())
    print("%d ticks of %d pendulums: mean |angle| %.2f -> %.2f rad, mean parameter error %.3f -> %.3f"
          % (a.ticks, a.envs, float(trace[0][:, 0].abs().mean()), float(trace[-1][:, 0].abs().mean()), err0, err1))
    return torch.stack(trace)


if __name__ == "__main__":
    main()
