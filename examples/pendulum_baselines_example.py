#!/usr/bin/env python3
"""The four cases of the reference's demo/pendulum_example.py:161-261, each as ONE batch on the device over the same true (length, mass)
rows - every episode of the demo is an environment:

    DuSt-MPC        SVMPC + the dynamics filter          run_pendulum_simulations            (BatchDualSVMPC.simulate)
    SVMPC           SVMPC, the prior's mean parameters   BatchSVMPC.simulate
    MPPI Baseline   MultiDISCO, one policy, exact model  run_pendulum_simulations(use_svmpc=False, use_exact_model=True)
    DISCO           MultiDISCO, one policy, sigma points run_pendulum_simulations(use_svmpc=False)   (BatchDISCO.simulate)

and the demo's figure of merit per case: AvgCumCost, the running mean of the cost, at the last period.  The plants step the controller's
model with g = 10 - the demo's stand-in for gym's Pendulum-v0 - under every episode's true parameters, without noise.

    python examples/pendulum_baselines_example.py --episodes 8 --steps 200
"""
import argparse
import os
import sys

import numpy as np
import torch
import torch.distributions as dist

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from pendulum_example import DEFAULTS, inst_cost, term_cost  # noqa: E402

from dust_amd.controllers import BatchDISCO, MultiDISCO  # noqa: E402
from dust_amd.inference import MPF, BatchSVMPC, ExponentiatedUtility, GaussianLikelihood, get_gmm  # noqa: E402
from dust_amd.kernels import RBFKernel  # noqa: E402
from dust_amd.models import PendulumModel  # noqa: E402
from dust_amd.utils.simulations import run_pendulum_simulations  # noqa: E402
from dust_amd.utils.utf import MerweScaledUTF  # noqa: E402

TINY = dict(episodes=3, steps=4, horizon=4, n_particles=2, action_samples=8, params_samples=2, mpf_n_particles=8, mpf_steps=2)
CASES = ("DuSt-MPC", "SVMPC", "MPPI Baseline", "DISCO")


def run(episodes=8, steps=200, seed=0, quiet=False, cases=CASES, **over):
    """-> {case: AvgCumCost [episodes, steps]}, the true (length, mass) [episodes, 2]"""
    e = dict(DEFAULTS["exp_params"], **over)
    torch.manual_seed(seed)
    B, N, H, S, M, alpha = episodes, e["n_particles"], e["horizon"], e["action_samples"], e["params_samples"], e["alpha"]
    env_model = PendulumModel()
    init_state = torch.as_tensor(e["init_state"]).clone()
    policies_prior = get_gmm(torch.randn(N, H, env_model.action_space.dim), torch.ones(N), e["prior_sigma"] ** 2 * torch.eye(e["ctrl_dim"]))
    init_policies = policies_prior.sample([N])
    dynamics_prior = dist.Independent(dist.Uniform(torch.tensor([0.6, 0.6]), torch.tensor([1.3, 1.3])), 1)
    true = dynamics_prior.sample([B])  # every episode its own (length, mass)
    truths = [dict(length=float(v[0]), mass=float(v[1])) for v in true]
    mean = dict(length=float(dynamics_prior.mean[0]), mass=float(dynamics_prior.mean[1]))
    ctrl_kwargs = dict(observation_space=env_model.observation_space, action_space=env_model.action_space, hz_len=H, action_samples=S,
                       temperature=1 / alpha, a_cov=e["ctrl_sigma"] ** 2 * torch.eye(e["ctrl_dim"]), inst_cost_fn=inst_cost, term_cost_fn=term_cost)
    seeds = [seed + b for b in range(B)]
    svmpc_kwargs = dict(init_particles=init_policies, prior=policies_prior, kernel=RBFKernel(), n_particles=N, bw_scale=e["bandwidth_scaling"],
                        n_steps=1, optimizer_class=torch.optim.SGD, lr=e["learning_rate"], weighted_prior=e["weighted_prior"], seeds=seeds)
    sampled = dict(g=10.0, uncertain_params=("length", "mass"))
    out = {}
    if "DuSt-MPC" in cases:
        controller = MultiDISCO(n_policies=N, params_samples=M, params_sampling=True, params_log_space=e["mpf_log_space"], **ctrl_kwargs)
        mpf_init = dynamics_prior.sample([B, e["mpf_n_particles"]])
        lik = GaussianLikelihood(initial_obs=init_state, obs_std=e["mpf_obs_std"], model=PendulumModel(uncertain_params=("length", "mass")),
                                 log_space=e["mpf_log_space"])
        mpf = MPF(init_particles=mpf_init[0], likelihood=lik, optimizer_class=torch.optim.SGD, lr=e["mpf_learning_rate"], bw=0.1,
                  bw_scale=e["mpf_bandwidth_scaling"])
        data = run_pendulum_simulations(init_state, init_policies, sampled, truths, controller, svmpc_kwargs, dict(alpha=alpha, n_samples=S), mpf,
                                        mpf_bw=e["mpf_bandwidth"], mpf_steps=e["mpf_steps"], episodes=B, steps=steps, warm_up=0, seed=seed,
                                        init_particles=mpf_init)
        out["DuSt-MPC"] = data["AvgCumCost"]
    if "SVMPC" in cases:
        # the prior's mean parameters in every rollout: one "sampled" row per period, which is that mean - so that the plants can still
        # step under the true rows
        controller = MultiDISCO(n_policies=N, params_samples=1, params_sampling=True, **ctrl_kwargs)
        controller.a_mat = init_policies.detach().clone()
        controller.return_rollouts = False
        model = PendulumModel(**sampled)
        sv = BatchSVMPC(B, likelihood=ExponentiatedUtility(alpha=alpha, n_samples=S, controller=controller, model=model), **svmpc_kwargs)
        rows = torch.tensor([mean["length"], mean["mass"]]).reshape(1, 1, 1, 1, 2).repeat(steps, B, 1, 1, 1)
        res = sv.simulate(init_state.reshape(1, -1).repeat(B, 1), dynamics_prior, steps, plant_params=true, params=rows)
        cost = res.costs.transpose(0, 1).numpy().astype(np.float64)
        out["SVMPC"] = np.round(np.cumsum(cost, 1) / (np.arange(steps) + 1), 2)
    if "MPPI Baseline" in cases:
        controller = BatchDISCO(B, n_policies=1, params_samples=1, params_sampling=True, seeds=seeds, **ctrl_kwargs)
        data = run_pendulum_simulations(init_state, init_policies[:1], sampled, truths, controller, None, None, None, episodes=B, steps=steps,
                                        use_svmpc=False, dyn_dist=dynamics_prior, use_exact_model=True)
        out["MPPI Baseline"] = data["AvgCumCost"]
    if "DISCO" in cases:
        controller = BatchDISCO(B, n_policies=1, params_sampling=MerweScaledUTF(n=2, alpha=0.5), params_log_space=False, seeds=seeds, **ctrl_kwargs)
        data = run_pendulum_simulations(init_state, init_policies[:1], dict(sampled, **mean), truths, controller, None, None, None, episodes=B,
                                        steps=steps, use_svmpc=False, dyn_dist=dynamics_prior)
        out["DISCO"] = data["AvgCumCost"]
    if not quiet:
        print("%d periods of %d pendulums per case; AvgCumCost at the last period" % (steps, B))
        print("  %-14s" % "episode" + "".join("%10d" % b for b in range(B)) + "%10s" % "mean")
        for k, v in out.items():
            print("  %-14s" % k + "".join("%10.2f" % x for x in v[:, -1]) + "%10.2f" % float(v[:, -1].mean()))
    return out, true


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--episodes", type=int, default=8)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--tiny", action="store_true", help="the size the test suite runs")
    a = ap.parse_args(argv)
    if a.tiny:
        return run(seed=a.seed, **TINY)
    return run(a.episodes, a.steps, seed=a.seed)


if __name__ == "__main__":
    main()
