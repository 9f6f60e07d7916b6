#!/usr/bin/env python3
"""B pendulum episodes at once: one `BatchSVMPC` - B independent SVMPC controllers whose tick is ONE kernel launch - against B host
plants, at the configuration of the reference's pendulum demo (3 Stein particles, 128 action samples, 8 dynamics samples, horizon 30,
one SVGD step per period).

The reference evaluates a controller over many episodes, each with a deep copy of the controller (dust/utils/simulations.py); here
the episodes run side by side.  Every episode has its own start state, its own true (length, mass), its own particles, prior and
noise stream; the model, the cost and the sizes are shared.  Per period:

    a_seq, p = controller.tick(states, params_dist) -> first action of every sequence to its plant

    python examples/svmpc_batch_example.py --envs 8 --steps 50
"""
import argparse
import os
import sys
import time

import torch
import torch.distributions as dist

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from dust_amd.controllers import MultiDISCO  # noqa: E402
from dust_amd.costs import PendulumQuadCos  # noqa: E402
from dust_amd.inference import BatchSVMPC, ExponentiatedUtility, get_gmm  # noqa: E402
from dust_amd.kernels import RBFKernel  # noqa: E402
from dust_amd.models import PendulumModel  # noqa: E402


def run(n_envs=8, steps=50, n_particles=3, n_samples=128, n_params=8, horizon=30, seed=0, quiet=False):
    """-> per-episode average cost [n_envs]"""
    torch.manual_seed(seed)
    cost = PendulumQuadCos()
    params_dist = dist.Independent(dist.Uniform(torch.tensor([0.6, 0.6]), torch.tensor([1.3, 1.3])), 1)  # (length, mass)
    model = PendulumModel(uncertain_params=("length", "mass"))
    true_params = params_dist.sample([n_envs])
    plants = [PendulumModel(g=10.0, length=float(p[0]), mass=float(p[1])) for p in true_params]
    states = torch.stack((torch.linspace(2.4, 3.6, n_envs), torch.zeros(n_envs)), 1)  # around the hanging position, at rest
    sigma2 = 4.0
    ctrl = MultiDISCO(model.observation_space, model.action_space, horizon, n_particles, n_samples, temperature=1.0,
                      a_cov=sigma2 * torch.eye(1), inst_cost_fn=cost.inst_cost, term_cost_fn=cost.term_cost, params_sampling=True,
                      params_samples=n_params, seed=seed)
    prior = get_gmm(torch.zeros(n_particles, horizon, 1), torch.ones(n_particles), sigma2 * torch.eye(1))
    init = prior.sample([n_envs, n_particles])  # [B, N, H, 1]: every episode starts from its own particles
    lik = ExponentiatedUtility(alpha=1.0, n_samples=n_samples, controller=ctrl, model=model)
    controller = BatchSVMPC(n_envs, init, prior, lik, kernel=RBFKernel(), n_particles=n_particles, n_steps=1,
                            optimizer_class=torch.optim.SGD, lr=1.0, seeds=[seed + b for b in range(n_envs)])
    total, t0 = torch.zeros(n_envs), time.perf_counter()
    for step in range(steps):
        a_seq, _ = controller.tick(states, params_dist)  # ONE launch for the B ticks
        actions = a_seq[:, 0]  # [B, da]
        states = torch.cat([plants[b].step(states[b:b + 1], actions[b].view(1, 1)) for b in range(n_envs)], 0)
        total += cost.inst_cost(states).reshape(n_envs)
        if not quiet and step % 20 == 0:
            print("step %3d  theta %s" % (step, " ".join("%+.2f" % float(v) for v in states[:, 0])))
    el = time.perf_counter() - t0
    avg = total / steps
    if not quiet:
        for b in range(n_envs):
            print("episode %2d  length %.2f mass %.2f  avg cost %8.2f" % (b, float(true_params[b, 0]), float(true_params[b, 1]), float(avg[b])))
        print("%d episodes x %d periods: %.1f environment-ticks/s incl. host plants" % (n_envs, steps, n_envs * steps / el))
    return avg


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=8)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--seed", type=int, default=0)
    args = ap.parse_args()
    run(args.envs, args.steps, seed=args.seed)


if __name__ == "__main__":
    main()
