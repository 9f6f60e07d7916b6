#!/usr/bin/env python3
"""A hyper-parameter sweep as ONE batch: B trials of the reference's pendulum tuning (demo/pendulum_tuning.py:30-143: one episode per
trial, each with its own lr, alpha - and temperature = 1 / alpha - and prior_sigma) are the B environments of a `BatchSVMPC`, and

    controller.set_hyper(lr=lr, alpha=alpha, temperature=1 / alpha, prior_sigma=prior_sigma)
    states, actions, p, a_seq = controller.run_episodes(states0, params_dist, steps, plant_params=true_params)

evaluates all of them in one kernel launch.  The search space is the script's - lr log-uniform in [0.1, 100], alpha uniform in [0.1, 10],
prior_sigma log-uniform in [0.1, 100] -, drawn here at random under a seed: the search strategy stays the caller's (the script's Optuna
would suggest the B rows of a round).  As in the script every trial meets the same plant, one true (length, mass) row drawn once, and
starts from the same state; the per-trial mean cost is computed on the host from the recorded states.  The horizon, the script's fourth
quantity, shapes the launch and is not per environment: a horizon sweep is one batch per value.

    python examples/svmpc_sweep_example.py --trials 64 --steps 50
    python examples/svmpc_sweep_example.py --tiny
"""
import argparse
import os
import sys
import time

import numpy as np
import torch
import torch.distributions as dist

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from dust_amd.controllers import MultiDISCO  # noqa: E402
from dust_amd.costs import PendulumQuadCos  # noqa: E402
from dust_amd.inference import BatchSVMPC, ExponentiatedUtility, get_gmm  # noqa: E402
from dust_amd.kernels import RBFKernel  # noqa: E402
from dust_amd.models import PendulumModel  # noqa: E402

TINY = dict(n_envs=4, steps=3, n_particles=2, n_samples=8, n_params=2, horizon=5)


def draw_rows(n, rng):
    """n rows of pendulum_tuning.py's search space; temperature = 1 / alpha is that script's line"""
    lr = np.exp(rng.uniform(np.log(1e-1), np.log(1e2), n))
    alpha = rng.uniform(1e-1, 1e1, n).astype(np.float32)
    prior_sigma = np.exp(rng.uniform(np.log(1e-1), np.log(1e2), n)).astype(np.float32)
    return dict(lr=lr, alpha=alpha, temperature=(1.0 / alpha).astype(np.float32), prior_sigma=prior_sigma)


def run(n_envs=64, steps=50, n_particles=3, n_samples=128, n_params=8, horizon=30, seed=0, quiet=False):
    """-> (per-trial mean cost [n_envs], the rows in force: `BatchSVMPC.hyper`)"""
    torch.manual_seed(seed)
    cost = PendulumQuadCos()
    params_dist = dist.Independent(dist.Uniform(torch.tensor([0.6, 0.6]), torch.tensor([1.3, 1.3])), 1)  # (length, mass)
    model = PendulumModel(uncertain_params=("length", "mass"))
    true_params = params_dist.sample([1]).repeat(n_envs, 1)  # one true row: all trials use the same plant
    states = torch.tensor([[3.0, 0.0]]).repeat(n_envs, 1)
    sigma2 = 4.0
    ctrl = MultiDISCO(model.observation_space, model.action_space, horizon, n_particles, n_samples, temperature=1.0,
                      a_cov=sigma2 * torch.eye(1), inst_cost_fn=cost.inst_cost, term_cost_fn=cost.term_cost, params_sampling=True,
                      params_samples=n_params, seed=seed)
    prior = get_gmm(torch.randn(n_particles, horizon, 1), torch.ones(n_particles), torch.eye(1))
    init = prior.sample([n_particles])
    lik = ExponentiatedUtility(alpha=1.0, n_samples=n_samples, controller=ctrl, model=model)
    controller = BatchSVMPC(n_envs, init, prior, lik, kernel=RBFKernel(), n_particles=n_particles, n_steps=1,
                            optimizer_class=torch.optim.SGD, lr=1.0, seeds=[seed + b for b in range(n_envs)])
    controller.set_hyper(**draw_rows(n_envs, np.random.default_rng(seed)))
    t0 = time.perf_counter()
    traj, _, _, _ = controller.run_episodes(states, params_dist, steps, plant_params=true_params)  # ONE launch: [T, B, ds]
    el = time.perf_counter() - t0
    avg = cost.inst_cost(traj.reshape(steps * n_envs, -1)).reshape(steps, n_envs).mean(0)
    rows = controller.hyper
    if not quiet:
        print("true length %.2f mass %.2f" % (float(true_params[0, 0]), float(true_params[0, 1])))
        for b in torch.argsort(avg)[:min(5, n_envs)].tolist():
            print("trial %3d  lr %8.3f  alpha %5.2f  prior_sigma %8.3f  mean cost %8.2f" % (b, rows["lr"][b], rows["alpha"][b], rows["sigma_p"][b, 0],
                                                                                        float(avg[b])))
        print("%d trials x %d periods in one launch: %.1f environment-ticks/s incl. the first call's set-up" % (n_envs, steps, n_envs * steps / el))
    return avg, rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--trials", type=int, default=64)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--tiny", action="store_true", help="4 trials of 3 periods at a small shape (what the test suite runs)")
    args = ap.parse_args()
    if args.tiny:
        run(seed=args.seed, **TINY)
    else:
        run(args.trials, args.steps, seed=args.seed)


if __name__ == "__main__":
    main()
