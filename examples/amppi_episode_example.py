#!/usr/bin/env python3
"""B pendulum episodes at once with the plants ON THE DEVICE: the pendulums of examples/amppi_batch_example.py, but every period -
update_actions, the plant's step with the first planned action, roll(1) - runs on the device, one kernel launch per period and no host
between two periods (`BatchAMPPI.run_episodes`, dust_amppi_batch_episode).

Every episode has its own start state, its own true (length, mass), its own nominal sequence and its own noise stream; the plants are
the controller's model under the episode's true parameters (every other constant is the model's), stepped without process noise.  The
episode runs in pieces of `--chunk` periods: each piece starts where the last one ended.

    python examples/amppi_episode_example.py --envs 8 --steps 50
    python examples/amppi_episode_example.py --tiny
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

TINY = dict(n_envs=4, steps=3, horizon=8, n_samples=64, chunk=2)


def run(n_envs=8, steps=50, horizon=30, n_samples=128, seed=0, chunk=25, quiet=False):
    """-> per-episode average cost [n_envs]"""
    torch.manual_seed(seed)
    cost = PendulumQuadCos()
    prior = dist.Independent(dist.Uniform(torch.tensor([0.6, 0.6]), torch.tensor([1.3, 1.3])), 1)
    model = PendulumModel(length=float(prior.mean[0]), mass=float(prior.mean[1]), uncertain_params=("length", "mass"))
    model.params_dist = prior
    true_params = prior.sample([n_envs])  # [B, P] in the columns of the controller's parameter rows
    states = torch.stack((torch.linspace(2.4, 3.6, n_envs), torch.zeros(n_envs)), 1)
    controller = BatchAMPPI(n_envs, model.observation_space, model.action_space, hz_len=horizon, n_samples=n_samples, lambda_=100.0,
                            a_cov=4.0 * torch.eye(1), inst_cost_fn=cost.inst_cost, term_cost_fn=cost.term_cost, params_sampling="extended",
                            seeds=[seed + b for b in range(n_envs)])
    total, done, t0 = torch.zeros(n_envs), 0, time.perf_counter()
    while done < steps:
        T = min(chunk, steps - done)
        xs, acts, _, _ = controller.run_episodes(model, states, T, plant_params=true_params)
        total += cost.inst_cost(xs.reshape(T * n_envs, -1)).reshape(T, n_envs).sum(0)
        states, done = xs[-1], done + T
        if not quiet:
            print("period %3d  theta %s" % (done, " ".join("%+.2f" % float(v) for v in states[:, 0])))
    el = time.perf_counter() - t0
    avg = total / steps
    if not quiet:
        for b in range(n_envs):
            print("episode %2d  length %.2f mass %.2f  avg cost %8.2f" % (b, float(true_params[b, 0]), float(true_params[b, 1]), float(avg[b])))
        print("%d episodes x %d periods: %.1f environment-periods/s incl. the parameter draws" % (n_envs, steps, n_envs * steps / el))
    return avg


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=8)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--horizon", type=int, default=30)
    ap.add_argument("--samples", type=int, default=128)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--chunk", type=int, default=25, help="periods per call")
    ap.add_argument("--tiny", action="store_true", help="the sizes the test suite runs")
    args = ap.parse_args()
    if args.tiny:
        run(**TINY)
    else:
        run(args.envs, args.steps, args.horizon, args.samples, args.seed, args.chunk)


if __name__ == "__main__":
    main()
