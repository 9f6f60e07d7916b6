#!/usr/bin/env python3
"""Skid-steer navigation round an occupancy grid with DuSt-MPC on the MI355X backend: a closed loop of SVMPC (the control side) and MPF
(the dynamics side, over the unknown x_icr) on `SkidSteerRobot`, driven by `dust_amd.costs.NavigationCost` - a quadratic cost to the goal
plus w_obs on every occupied cell of one of `get_obst_preset`'s maps.  The plant is the host `SkidSteerRobot.step` with the true x_icr.
The reference ships no skid-steer demo; the loop is the one of its simulations (dust/utils/simulations.py:104-138) as `DualSVMPC` runs it.

    python examples/skid_steer_example.py --ticks 100
"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from dust_amd.controllers import DualSVMPC, MultiDISCO  # noqa: E402
from dust_amd.costs import NavigationCost  # noqa: E402
from dust_amd.inference import MPF, SVMPC, ExponentiatedUtility, GaussianLikelihood, get_gmm  # noqa: E402
from dust_amd.kernels import RBFKernel  # noqa: E402
from dust_amd.models import SkidSteerRobot  # noqa: E402
from dust_amd.utils.obstacle_map import generate_obstacle_map, get_obst_preset  # noqa: E402


def main(argv=None):
    """-> the plant's states [ticks + 1, 5]"""
    ap = argparse.ArgumentParser()
    ap.add_argument("--horizon", type=int, default=20)
    ap.add_argument("--ticks", type=int, default=100)
    ap.add_argument("--particles", type=int, default=8, help="Stein particles of the control side")
    ap.add_argument("--samples", type=int, default=32, help="action samples per particle")
    ap.add_argument("--params", type=int, default=4, help="dynamics samples per rollout")
    ap.add_argument("--mpf-particles", type=int, default=64)
    ap.add_argument("--preset", default="grid_6x6")
    ap.add_argument("--w-obs", type=float, default=20.0)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--verbose", action="store_true")
    a = ap.parse_args(argv)
    torch.manual_seed(a.seed)
    N, S, M, H, dt, sigma = a.particles, a.samples, a.params, a.horizon, 0.1, 1.0
    obst_map = generate_obstacle_map(map_dim=(22, 22), obst_list=get_obst_preset(a.preset, obst_width=1.0), cell_size=0.1, map_type="direct")
    start, goal = torch.tensor([-2.9, -2.6, 0.6, 0.0, 0.0]), (2.6, 2.9, 0.0, 0.0, 0.0)
    cost = NavigationCost(goal, (1.0, 1.0, 0.0, 0.0, 0.0), (20.0, 20.0, 0.0, 0.0, 0.0), (0.01, 0.01), obst_map=obst_map, w_obs=a.w_obs)
    model = SkidSteerRobot(delta_t=dt, uncertain_params=("x_icr",), min_wheel_speed=-3.0, max_wheel_speed=3.0)
    plant = SkidSteerRobot(delta_t=dt, x_icr=0.3, min_wheel_speed=-3.0, max_wheel_speed=3.0)  # the true robot: x_icr 0.3, the model believes 0.2
    ctrl = MultiDISCO(observation_space=model.observation_space, action_space=model.action_space, hz_len=H, n_policies=N, action_samples=S,
                      params_samples=M, temperature=5.0, a_cov=sigma ** 2 * torch.eye(2), inst_cost_fn=cost.inst_cost, term_cost_fn=cost.term_cost,
                      params_sampling=True, params_log_space=True, seed=a.seed)
    mu0 = 1.5 + 0.5 * torch.randn(N, H, 2)
    theta0 = mu0 + 0.3 * torch.randn(N, H, 2)
    ctrl.a_mat = theta0.clone()
    ctrl.return_rollouts = False
    svmpc = SVMPC(likelihood=ExponentiatedUtility(alpha=0.2, n_samples=S, controller=ctrl, model=model), init_particles=theta0.clone(),
                  prior=get_gmm(mu0, torch.ones(N), sigma ** 2 * torch.eye(2)), kernel=RBFKernel(), n_particles=N, bw_scale=1.0, n_steps=1,
                  optimizer_class=torch.optim.SGD, lr=0.5)
    x0 = (torch.tensor(0.2).log() + 0.3 * torch.randn(a.mpf_particles, 1))
    mpf = MPF(init_particles=x0, likelihood=GaussianLikelihood(initial_obs=start, obs_std=0.05, model=model, log_space=True),
              optimizer_class=torch.optim.SGD, lr=1e-3, bw=0.3, bw_scale=1.0)
    loop = DualSVMPC(svmpc, mpf, mpf_bw=0.3, mpf_steps=10, warm_up=0, fused=True, seed=a.seed)
    state, states, hits = start.reshape(1, -1), [start.clone()], 0
    for t in range(a.ticks):
        action, state, _ = loop.tick(state, lambda x, u: plant.step(x.reshape(1, -1), u.reshape(1, -1)))
        states.append(state.reshape(-1).clone())
        hits += int(obst_map.get_collisions(state.reshape(1, -1)[:, 0:2]).item())
        if a.verbose:
            print("tick %3d  action (%+.2f, %+.2f)  state (%+.2f, %+.2f, %+.2f)" % ((t,) + tuple(action.tolist()) + tuple(state.reshape(-1)[:3].tolist())))
    states = torch.stack(states)
    d0, d1 = (float((x[:2] - torch.tensor(goal[:2])).norm()) for x in (states[0], states[-1]))
    print("%d ticks: distance to the goal %.2f -> %.2f m, %d steps on occupied cells, x_icr estimate %.3f (true 0.300)"
          % (a.ticks, d0, d1, hits, float(loop.dyn_particles.exp().mean())))
    return states


if __name__ == "__main__":
    main()
