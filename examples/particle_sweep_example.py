#!/usr/bin/env python3
"""The point-mass tuning sweep as ONE batch: B trials of the reference's demo/particle_tuning.py - one episode of `run_particle_episode`
per trial, each with its own lr, alpha (temperature = 1 / alpha), prior_sigma, prior_weighted and ctrl_sigma - are the B environments of a
`BatchSVMPC`, and

    controller.set_hyper(lr=lr, alpha=alpha, temperature=1 / alpha, prior_sigma=prior_sigma, ctrl_sigma=ctrl_sigma, weighted_prior=w)
    losses = run_particle_episodes(states0, model, dynamics_prior, controller, warm_up=30, steps=400)

runs the reference's episode for all of them on the device - warm-up, the accumulated cost, the crash that costs inf, the stop within
1.0 of the target - and returns the B losses the script minimises, so the trials rank as they do there.  The search space is the
script's - lr log-uniform in [0.1, 100], alpha log-uniform in [0.1, 10], prior_sigma log-uniform in [1, 100], prior_weighted 0 / 1,
ctrl_sigma uniform in [1, 100] -, drawn here at random under a seed: the search strategy stays the caller's.  The horizon, the script's
sixth quantity, shapes the launch and is not per environment: a horizon sweep is one batch per value.  The plants are deterministic.

    python examples/particle_sweep_example.py --trials 64 --steps 400
    python examples/particle_sweep_example.py --tiny
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
from dust_amd.inference import BatchSVMPC, ExponentiatedUtility, get_gmm  # noqa: E402
from dust_amd.kernels import RBFKernel  # noqa: E402
from dust_amd.models import Particle  # noqa: E402
from dust_amd.utils.simulations import run_particle_episodes  # noqa: E402

ENV = dict(dt=0.015, control_type="acceleration", noise_std=[0.1, 0.1], init_state=[-9.0, -9.0, 0, 0], target_state=[9.0, 9.0, 0, 0],
           can_crash=True, with_obstacle=True, deterministic=True,
           cost_params=dict(w_qpos=0.5, w_qvel=0.25, w_ctrl=0.2, w_obs=1.0e6, w_qpos_T=1.0e3, w_qvel_T=0.1),
           obst_preset="grid_4x4", obst_width=2.1, max_speed=5, max_accel=10, map_cell_size=0.1, map_size=[22, 22], map_type="direct")
TINY = dict(n_trials=4, steps=6, warm_up=2, n_particles=2, n_samples=8, n_params=2, horizon=5)


def draw_rows(n, rng):
    """n rows of particle_tuning.py's search space; temperature = 1 / alpha is that script's line"""
    lr = np.exp(rng.uniform(np.log(1e-1), np.log(1e2), n))
    alpha = np.exp(rng.uniform(np.log(1e-1), np.log(1e1), n)).astype(np.float32)
    prior_sigma = np.exp(rng.uniform(np.log(1.0), np.log(1e2), n)).astype(np.float32)
    return dict(lr=lr, alpha=alpha, temperature=(1.0 / alpha).astype(np.float32), prior_sigma=prior_sigma,
                weighted_prior=rng.integers(0, 2, n), ctrl_sigma=rng.uniform(1.0, 1e2, n).astype(np.float32))


def run(n_trials=64, steps=400, warm_up=30, n_particles=6, n_samples=64, n_params=4, horizon=20, seed=0, quiet=False):
    """-> (losses [n_trials], the trials ordered by loss: dicts of a trial's row and its loss)"""
    torch.manual_seed(seed)
    dynamics_prior = dist.Normal(2.0, 0.1)
    model = Particle(**ENV, uncertain_params=["mass"], mass=dynamics_prior.mean)
    ctrl = MultiDISCO(model.observation_space, model.action_space, horizon, n_particles, n_samples, temperature=1.0, a_cov=25.0 * torch.eye(2),
                      inst_cost_fn=model.default_inst_cost, term_cost_fn=model.default_term_cost, params_sampling=True, params_samples=n_params,
                      seed=seed)
    prior = get_gmm(torch.randn(n_particles, horizon, 2), torch.ones(n_particles), 25.0 * torch.eye(2))
    init = prior.sample([n_particles])
    lik = ExponentiatedUtility(alpha=1.0, n_samples=n_samples, controller=ctrl, model=model)
    controller = BatchSVMPC(n_trials, init, prior, lik, kernel=RBFKernel(), n_particles=n_particles, n_steps=1, optimizer_class=torch.optim.SGD,
                            lr=1.0, seeds=[seed + b for b in range(n_trials)])
    controller.set_hyper(**draw_rows(n_trials, np.random.default_rng(seed)))
    states = torch.as_tensor(ENV["init_state"], dtype=torch.float).repeat(n_trials, 1)
    t0 = time.perf_counter()
    losses = run_particle_episodes(states, model, dynamics_prior, controller, warm_up=warm_up, steps=steps)  # one launch per piece
    el = time.perf_counter() - t0
    rows = controller.hyper
    order = sorted(range(n_trials), key=lambda b: float(losses[b]))
    table = [dict(trial=b, lr=float(rows["lr"][b]), alpha=float(rows["alpha"][b]), prior_sigma=float(rows["sigma_p"][b, 0]),
                  ctrl_sigma=float(rows["sigma_a"][b, 0]), prior_weighted=int(rows["weighted_prior"][b]), loss=float(losses[b])) for b in order]
    if not quiet:
        for r in table[:min(5, n_trials)]:
            print("trial %(trial)3d  lr %(lr)8.3f  alpha %(alpha)5.2f  prior_sigma %(prior_sigma)7.2f  ctrl_sigma %(ctrl_sigma)6.2f  "
                  "prior_weighted %(prior_weighted)d  loss %(loss)12.4g" % r)
        print("%d trials x up to %d periods: %.2f s incl. the first call's set-up" % (n_trials, steps, el))
    return losses, table


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--trials", type=int, default=64)
    ap.add_argument("--steps", type=int, default=400)
    ap.add_argument("--warm-up", type=int, default=30)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--tiny", action="store_true", help="4 trials of 6 periods at a small shape (what the test suite runs)")
    args = ap.parse_args()
    if args.tiny:
        run(seed=args.seed, **TINY)
    else:
        run(args.trials, args.steps, args.warm_up, seed=args.seed)


if __name__ == "__main__":
    main()
