#!/usr/bin/env python3
"""The episodes of examples/pendulum_example.py --case dual as ONE batch on the device: `run_pendulum_simulations`, the batched twin of
`run_pendulum_simulation(use_svmpc=True, mpf=...)`.  Every episode is an environment of one `BatchSVMPC` plus `BatchDualSVMPC` with its
own true (length, mass); the whole loop of dust/utils/simulations.py:104-138 - warm-up periods that only optimize and apply a zero
torque while the filters keep updating, the tick, the plant's step, the cost of the new state, the filter's conditioning - runs in one
C call per episode piece (dust_svmpc_dual_batch_simulate), with no host round trip between the periods.

The objects are built with the demo's arguments (3 Stein particles, 128 action samples, 8 dynamics samples, horizon 30, one SVGD step
per period, SGD with lr 2, 50 filter particles, 20 filter steps).  The plants step the controller's own model with g = 10 - the demo's
stand-in for gym's Pendulum-v0 - under every episode's true parameters.

    python examples/pendulum_dual_sim_example.py --episodes 8 --steps 200 --warm-up 10
"""
import argparse
import os
import sys

import torch
import torch.distributions as dist

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from pendulum_example import DEFAULTS, inst_cost, term_cost  # noqa: E402

from dust_amd.controllers import MultiDISCO  # noqa: E402
from dust_amd.inference import MPF, GaussianLikelihood, get_gmm  # noqa: E402
from dust_amd.kernels import RBFKernel  # noqa: E402
from dust_amd.models import PendulumModel  # noqa: E402
from dust_amd.utils.simulations import run_pendulum_simulations  # noqa: E402

TINY = dict(episodes=3, steps=5, warm_up=2, horizon=4, n_particles=2, action_samples=8, params_samples=2, mpf_n_particles=8, mpf_steps=2)


def run(episodes=8, steps=200, warm_up=10, seed=0, quiet=False, history=False, **over):
    """-> (the dict of run_pendulum_simulations, the true (length, mass) [B, 2]); history: one DynParticles / PolParticles row per period"""
    e = dict(DEFAULTS["exp_params"], **over)
    torch.manual_seed(seed)
    N, H, S, M, alpha = e["n_particles"], e["horizon"], e["action_samples"], e["params_samples"], e["alpha"]
    env_model = PendulumModel()
    init_state = torch.as_tensor(e["init_state"]).clone()
    policies_prior = get_gmm(torch.randn(N, H, env_model.action_space.dim), torch.ones(N), e["prior_sigma"] ** 2 * torch.eye(e["ctrl_dim"]))
    init_policies = policies_prior.sample([N])
    dynamics_prior = dist.Independent(dist.Uniform(torch.tensor([0.6, 0.6]), torch.tensor([1.3, 1.3])), 1)
    true = dynamics_prior.sample([episodes])  # every episode its own (length, mass)
    controller = MultiDISCO(observation_space=env_model.observation_space, action_space=env_model.action_space, hz_len=H, n_policies=N,
                            action_samples=S, params_samples=M, temperature=1 / alpha, a_cov=e["ctrl_sigma"] ** 2 * torch.eye(e["ctrl_dim"]),
                            inst_cost_fn=inst_cost, term_cost_fn=term_cost, params_sampling=True, params_log_space=e["mpf_log_space"])
    mpf_init = dynamics_prior.sample([episodes, e["mpf_n_particles"]])  # ... and its own belief to start from
    lik = GaussianLikelihood(initial_obs=init_state, obs_std=e["mpf_obs_std"], model=PendulumModel(uncertain_params=("length", "mass")),
                             log_space=e["mpf_log_space"])
    mpf = MPF(init_particles=mpf_init[0], likelihood=lik, optimizer_class=torch.optim.SGD, lr=e["mpf_learning_rate"], bw=0.1,
              bw_scale=e["mpf_bandwidth_scaling"])
    svmpc_kwargs = dict(init_particles=init_policies, prior=policies_prior, kernel=RBFKernel(), n_particles=N, bw_scale=e["bandwidth_scaling"],
                        n_steps=1, optimizer_class=torch.optim.SGD, lr=e["learning_rate"], weighted_prior=e["weighted_prior"],
                        seeds=[seed + b for b in range(episodes)])
    data = run_pendulum_simulations(init_state, init_policies, dict(g=10.0, uncertain_params=("length", "mass")),
                                    [dict(length=float(v[0]), mass=float(v[1])) for v in true], controller, svmpc_kwargs,
                                    dict(alpha=alpha, n_samples=S), mpf, mpf_bw=e["mpf_bandwidth"], mpf_steps=e["mpf_steps"], episodes=episodes,
                                    steps=steps, warm_up=warm_up, seed=seed, init_particles=mpf_init, history=history)
    if not quiet:
        est = (data["DynParticles"][:, -1] if history else data["DynParticles"]).mean(1)
        print("%d periods of %d pendulums, %d of them warm-up: final mean |angle| %.2f rad"
              % (steps, episodes, min(warm_up, steps), float(abs(data["Position"][:, -1]).mean())))
        for b in range(episodes):
            print("  episode %2d  AvgCumCost %9.2f   length %.3f (true %.3f)   mass %.3f (true %.3f)"
                  % (b, data["AvgCumCost"][b, -1], est[b, 0], float(true[b, 0]), est[b, 1], float(true[b, 1])))
    return data, true


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--episodes", type=int, default=8)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warm-up", type=int, default=10)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--tiny", action="store_true", help="the size the test suite runs")
    a = ap.parse_args(argv)
    if a.tiny:
        return run(seed=a.seed, **TINY)
    return run(a.episodes, a.steps, a.warm_up, seed=a.seed)


if __name__ == "__main__":
    main()
