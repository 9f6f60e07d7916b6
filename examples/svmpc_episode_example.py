#!/usr/bin/env python3
"""B pendulum episodes at once with the plants on the device: the scenario of examples/svmpc_batch_example.py - the reference's pendulum
demo (3 Stein particles, 128 action samples, 8 dynamics samples, horizon 30, one SVGD step per period), every episode with its own
start state, true (length, mass), particles, prior and noise stream - run by ONE call and ONE kernel launch for the whole episode:

    states, actions, p, a_seq = controller.run_episodes(states0, params_dist, steps, plant_params=true_params)

Per period the kernel runs the tick, steps the plant with the first action of the chosen sequence under the episode's true parameters
and feeds the new state to the next tick (dust/utils/simulations.py:104-130); the recorded states come back once, and the per-episode
average cost is computed from them on the host.  One difference from the host-plant example: a device plant is the controller's own
model at other parameter values, so its g is the model's 9.8 (the host plants there are built with g = 10).

    python examples/svmpc_episode_example.py --envs 8 --steps 50
    python examples/svmpc_episode_example.py --tiny
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

TINY = dict(n_envs=3, steps=4, n_particles=2, n_samples=8, n_params=2, horizon=5)


def run(n_envs=8, steps=50, n_particles=3, n_samples=128, n_params=8, horizon=30, seed=0, quiet=False):
    """-> per-episode average cost [n_envs]"""
    torch.manual_seed(seed)
    cost = PendulumQuadCos()
    params_dist = dist.Independent(dist.Uniform(torch.tensor([0.6, 0.6]), torch.tensor([1.3, 1.3])), 1)  # (length, mass)
    model = PendulumModel(uncertain_params=("length", "mass"))
    true_params = params_dist.sample([n_envs])  # [B, 2]: every plant's own (length, mass)
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
    t0 = time.perf_counter()
    traj, _, _, _ = controller.run_episodes(states, params_dist, steps, plant_params=true_params)  # ONE launch: [T, B, ds]
    el = time.perf_counter() - t0
    avg = cost.inst_cost(traj.reshape(steps * n_envs, -1)).reshape(steps, n_envs).mean(0)
    if not quiet:
        for step in range(0, steps, 20):
            print("step %3d  theta %s" % (step, " ".join("%+.2f" % float(v) for v in traj[step, :, 0])))
        for b in range(n_envs):
            print("episode %2d  length %.2f mass %.2f  avg cost %8.2f" % (b, float(true_params[b, 0]), float(true_params[b, 1]), float(avg[b])))
        print("%d episodes x %d periods in one launch: %.1f environment-ticks/s incl. the first call's set-up" % (n_envs, steps, n_envs * steps / el))
    return avg


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=8)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--tiny", action="store_true", help="3 episodes of 4 periods at a small shape (what the test suite runs)")
    args = ap.parse_args()
    if args.tiny:
        run(seed=args.seed, **TINY)
    else:
        run(args.envs, args.steps, seed=args.seed)


if __name__ == "__main__":
    main()
