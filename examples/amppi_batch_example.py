#!/usr/bin/env python3
"""B pendulum episodes at once: one `BatchAMPPI` - B independent AMPPI controllers ticking in ONE kernel launch - against B host plants.

The reference evaluates a controller over many episodes, each with its own deep copy (dust/utils/simulations.py); here the episodes
run side by side.  Every episode has its own start state, its own true (length, mass), its own nominal sequence and its own noise
stream; the model, the cost, the horizon and the number of samples are shared.  Per period:

    controller.update_actions(model, states) -> first action of every sequence to its plant -> controller.roll(1)

    python examples/amppi_batch_example.py --envs 8 --steps 50
"""
import argparse
import os
import sys
import time

import torch
import torch.distributions as dist

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from dust_amd.controllers import BatchAMPPI  # noqa: E402
from dust_amd.costs import PendulumQuadCos  # noqa: E402
from dust_amd.models import PendulumModel  # noqa: E402


def run(n_envs=8, steps=50, horizon=30, n_samples=128, seed=0, quiet=False):
    """-> per-episode average cost [n_envs]"""
    torch.manual_seed(seed)
    cost = PendulumQuadCos()
    prior = dist.Independent(dist.Uniform(torch.tensor([0.6, 0.6]), torch.tensor([1.3, 1.3])), 1)
    model = PendulumModel(length=float(prior.mean[0]), mass=float(prior.mean[1]), uncertain_params=("length", "mass"))
    model.params_dist = prior
    true_params = prior.sample([n_envs])
    plants = [PendulumModel(g=10.0, length=float(p[0]), mass=float(p[1])) for p in true_params]
    # start states spread around the hanging position, at rest
    states = torch.stack((torch.linspace(2.4, 3.6, n_envs), torch.zeros(n_envs)), 1)
    # lambda_ = 100: the pendulum's costs run into the hundreds (examples/pendulum_example.py --case amppi)
    controller = BatchAMPPI(n_envs, model.observation_space, model.action_space, hz_len=horizon, n_samples=n_samples, lambda_=100.0,
                            a_cov=4.0 * torch.eye(1), inst_cost_fn=cost.inst_cost, term_cost_fn=cost.term_cost, params_sampling="extended",
                            seeds=[seed + b for b in range(n_envs)])
    controller.return_rollouts = False
    total, t0 = torch.zeros(n_envs), time.perf_counter()
    for step in range(steps):
        controller.update_actions(model, states)
        actions = controller.a_seq[:, 0]  # [B, da]
        states = torch.cat([plants[b].step(states[b:b + 1], actions[b].view(1, 1)) for b in range(n_envs)], 0)
        controller.roll(1)
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
    ap.add_argument("--horizon", type=int, default=30)
    ap.add_argument("--samples", type=int, default=128)
    ap.add_argument("--seed", type=int, default=0)
    args = ap.parse_args()
    run(args.envs, args.steps, args.horizon, args.samples, args.seed)


if __name__ == "__main__":
    main()
