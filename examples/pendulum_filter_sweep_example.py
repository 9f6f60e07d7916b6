#!/usr/bin/env python3
"""A sweep over the dynamics FILTER's settings as ONE batch on the device: the four lines of the reference's demo/pendulum_config.yaml
that its own tuning scripts do not reach - mpf_learning_rate, mpf_obs_std, mpf_bandwidth, mpf_bandwidth_scaling - drawn log-uniformly
for B trials, every trial an environment of one `BatchSVMPC` plus `BatchDualSVMPC` (`run_pendulum_simulations(mpf_hyper=...)`,
`BatchDualSVMPC.set_filter_hyper`, dust_mpf_batch_set_hyper).  All trials share the plant's true (length, mass), the controller and the
filter's first particles: they differ in their filter rows alone.  Half of the trials fix the kernel bandwidth, the others take
Silverman's rule on their own particles times their bandwidth scaling.

Per trial: AvgCumCost of the episode and the error of the filter's mean estimate against the true (length, mass); the best rows by cost
are printed.

    python examples/pendulum_filter_sweep_example.py --trials 64 --steps 200 --warm-up 10
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

from dust_amd.controllers import MultiDISCO  # noqa: E402
from dust_amd.inference import MPF, GaussianLikelihood, get_gmm  # noqa: E402
from dust_amd.kernels import RBFKernel  # noqa: E402
from dust_amd.models import PendulumModel  # noqa: E402
from dust_amd.utils.simulations import run_pendulum_simulations  # noqa: E402

TINY = dict(trials=4, steps=5, warm_up=2, horizon=4, n_particles=2, action_samples=8, params_samples=2, mpf_n_particles=8, mpf_steps=2)
# log-uniform ranges around the demo's values
RANGES = dict(lr=(1e-4, 1e-2), obs_std=(0.05, 0.5), bw_scale=(0.25, 4.0), bw=(0.02, 0.5))


def draw_rows(trials, rng):
    """B filter rows: lr, obs_std and bw_scale log-uniform; every other trial a fixed bandwidth (log-uniform), the rest Silverman's rule"""
    def lu(k):
        lo, hi = RANGES[k]
        return float(np.exp(rng.uniform(np.log(lo), np.log(hi))))

    return [dict(lr=lu("lr"), obs_std=lu("obs_std"), bw_scale=lu("bw_scale"), bw=lu("bw") if b % 2 else 0.0) for b in range(trials)]


def run(trials=64, steps=200, warm_up=10, seed=0, quiet=False, true=(0.8, 1.2), **over):
    """-> (the dict of run_pendulum_simulations, the rows, the estimates' errors [B])"""
    e = dict(DEFAULTS["exp_params"], **over)
    torch.manual_seed(seed)
    B = int(trials)
    N, H, S, M, alpha = e["n_particles"], e["horizon"], e["action_samples"], e["params_samples"], e["alpha"]
    env_model = PendulumModel()
    init_state = torch.as_tensor(e["init_state"]).clone()
    policies_prior = get_gmm(torch.randn(N, H, env_model.action_space.dim), torch.ones(N), e["prior_sigma"] ** 2 * torch.eye(e["ctrl_dim"]))
    init_policies = policies_prior.sample([N])
    dynamics_prior = dist.Independent(dist.Uniform(torch.tensor([0.6, 0.6]), torch.tensor([1.3, 1.3])), 1)
    controller = MultiDISCO(observation_space=env_model.observation_space, action_space=env_model.action_space, hz_len=H, n_policies=N,
                            action_samples=S, params_samples=M, temperature=1 / alpha, a_cov=e["ctrl_sigma"] ** 2 * torch.eye(e["ctrl_dim"]),
                            inst_cost_fn=inst_cost, term_cost_fn=term_cost, params_sampling=True, params_log_space=e["mpf_log_space"])
    mpf_init = dynamics_prior.sample([e["mpf_n_particles"]])
    if e["mpf_log_space"]:
        mpf_init = mpf_init.log()
    lik = GaussianLikelihood(initial_obs=init_state, obs_std=e["mpf_obs_std"], model=PendulumModel(uncertain_params=("length", "mass")),
                             log_space=e["mpf_log_space"])
    mpf = MPF(init_particles=mpf_init, likelihood=lik, optimizer_class=torch.optim.SGD, lr=e["mpf_learning_rate"], bw=0.1,
              bw_scale=e["mpf_bandwidth_scaling"])
    svmpc_kwargs = dict(init_particles=init_policies, prior=policies_prior, kernel=RBFKernel(), n_particles=N, bw_scale=e["bandwidth_scaling"],
                        n_steps=1, optimizer_class=torch.optim.SGD, lr=e["learning_rate"], weighted_prior=e["weighted_prior"],
                        seeds=[seed] * B)  # (the same noise in every trial: the rows are the only difference)
    rows = draw_rows(B, np.random.default_rng(seed))
    data = run_pendulum_simulations(init_state, init_policies, dict(g=10.0, uncertain_params=("length", "mass")),
                                    [dict(length=float(true[0]), mass=float(true[1]))] * B, controller, svmpc_kwargs,
                                    dict(alpha=alpha, n_samples=S), mpf, mpf_bw=None, mpf_steps=e["mpf_steps"], episodes=B, steps=steps,
                                    warm_up=warm_up, seed=seed, init_particles=mpf_init[None].repeat(B, 1, 1), mpf_hyper=rows)
    x = data["DynParticles"]
    est = (np.exp(x) if e["mpf_log_space"] else x).mean(1)
    err = np.abs(est - np.asarray(true, np.float32)[None]).max(1)
    cost = data["AvgCumCost"][:, -1]
    if not quiet:
        print("%d trials of %d periods (%d warm-up), true (length, mass) = (%.2f, %.2f)" % (B, steps, min(warm_up, steps), true[0], true[1]))
        print("best rows by AvgCumCost:")
        for b in np.argsort(np.where(np.isfinite(cost), cost, np.inf))[:min(B, 5)]:
            r = rows[b]
            print("  trial %3d  AvgCumCost %9.2f  |estimate - true| %.3f   lr %.2e  obs_std %.3f  %s"
                  % (b, cost[b], err[b], r["lr"], r["obs_std"], "bw %.3f" % r["bw"] if r["bw"] > 0 else "Silverman x %.2f" % r["bw_scale"]))
    return data, rows, err


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--trials", type=int, default=64)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warm-up", type=int, default=10)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--tiny", action="store_true", help="the size the test suite runs")
    a = ap.parse_args(argv)
    if a.tiny:
        return run(seed=a.seed, **TINY)
    return run(a.trials, a.steps, a.warm_up, seed=a.seed)


if __name__ == "__main__":
    main()
