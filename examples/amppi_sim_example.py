#!/usr/bin/env python3
"""B Particle navigation episodes under AMPPI with the plants, the cost and the stops ON THE DEVICE: the `use_svmpc=False` branch of the
reference's run_particle_episode - update_actions, the plant's step, the accumulated cost, a crash that costs inf, a stop inside the goal
radius, roll(1) - for B plants in one `run_particle_episodes` call (`BatchAMPPI.simulate`, dust_amppi_batch_simulate): one kernel launch
per period and no host between two periods.

Every episode has its own start on the `grid_4x4` map of `get_obst_preset`, its own true mass and its own noise stream; the plants step
without process noise.  Prints the losses, the statuses (0 still running, 1 goal, 2 crash) and the periods every episode ran.

    python examples/amppi_sim_example.py --envs 8 --steps 200
    python examples/amppi_sim_example.py --tiny
"""
import argparse
import os
import sys

import torch
import torch.distributions as dist

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from dust_amd.controllers import BatchAMPPI  # noqa: E402
from dust_amd.models import Particle  # noqa: E402
from dust_amd.utils.simulations import run_particle_episodes  # noqa: E402

TINY = dict(n_envs=4, steps=4, horizon=8, n_samples=64)
COST = dict(w_qpos=0.01, w_qvel=1.0, w_ctrl=0.2, w_obs=20.0, w_qpos_T=0.1, w_qvel_T=1.0)


def run(n_envs=8, steps=200, horizon=20, n_samples=256, seed=0, quiet=False):
    """-> (losses [n_envs], statuses [n_envs], periods run [n_envs])"""
    torch.manual_seed(seed)
    model = Particle(dt=0.015, control_type="acceleration", noise_std=[0.1, 0.1], init_state=[-9.0, -9.0, 0.0, 0.0], target_state=[9.0, 9.0, 0.0, 0.0],
                     can_crash=True, with_obstacle=True, deterministic=True, cost_params=COST, obst_preset="grid_4x4", obst_width=2.1, max_speed=5,
                     max_accel=10, map_cell_size=0.1, map_size=[22, 22], map_type="direct", mass=2.0, uncertain_params=("mass",))
    model.params_dist = dist.Independent(dist.Uniform(torch.tensor([1.5]), torch.tensor([2.5])), 1)
    true_mass = model.params_dist.sample([n_envs])  # [B, 1] in the column of the controller's parameter rows
    # starts along the lower-left corridor of the map, and one inside the goal radius
    states = torch.zeros(n_envs, 4)
    states[:, 0] = torch.linspace(-9.5, -8.5, n_envs)
    states[:, 1] = torch.linspace(-8.5, -9.5, n_envs)
    states[-1] = torch.tensor([8.8, 8.9, 0.1, -0.1])
    controller = BatchAMPPI(n_envs, model.observation_space, model.action_space, hz_len=horizon, n_samples=n_samples, lambda_=50.0,
                            a_cov=25.0 * torch.eye(2), inst_cost_fn=model.default_inst_cost, term_cost_fn=model.default_term_cost,
                            params_sampling="extended", seeds=[seed + b for b in range(n_envs)])
    losses, status, n_run = run_particle_episodes(states, model, None, controller, steps=steps, plant_params=true_mass, details=True)
    if not quiet:
        for b in range(n_envs):
            print("episode %2d  mass %.2f  loss %10.3f  status %d  periods %d" % (b, float(true_mass[b, 0]), float(losses[b]), int(status[b]), int(n_run[b])))
    return losses, status, n_run


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=8)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--horizon", type=int, default=20)
    ap.add_argument("--samples", type=int, default=256)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--tiny", action="store_true", help="the sizes the test suite runs")
    args = ap.parse_args()
    if args.tiny:
        run(**TINY)
    else:
        run(args.envs, args.steps, args.horizon, args.samples, args.seed)


if __name__ == "__main__":
    main()
