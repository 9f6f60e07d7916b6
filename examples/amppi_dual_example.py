#!/usr/bin/env python3
"""The dual loop over an AMPPI controller on the MI355X backend: `AMPPI` (the control side, one kernel launch per tick) and `MPF` (the
dynamics side, over the unknown wheel radius) on `SkidSteerRobot`, driven by `dust_amd.costs.NavigationCost` on one of `get_obst_preset`'s
maps.  The plant is the host `SkidSteerRobot.step` with the TRUE wheel radius; the controller starts from another belief and the filter
recovers it.  `DualAMPPI(fused=True)` runs a control period - filter update, parameter draws inside the tick's kernel, update, roll - in
one C call.  The loop is the one of the reference's simulations (dust/utils/simulations.py:104-138) with dust/controllers/amppi.py:227-260
as the controller.

    python examples/amppi_dual_example.py --ticks 100
"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from dust_amd.controllers import AMPPI, DualAMPPI  # noqa: E402
from dust_amd.costs import NavigationCost  # noqa: E402
from dust_amd.inference import MPF, GaussianLikelihood  # noqa: E402
from dust_amd.models import SkidSteerRobot  # noqa: E402
from dust_amd.utils.obstacle_map import generate_obstacle_map, get_obst_preset  # noqa: E402

TRUE_RADIUS, BELIEF = 0.08, 0.0625


def scenario(samples=1024, horizon=20, mpf_particles=64, preset="grid_6x6", w_obs=20.0, seed=0, fused=True, sampling="extended", mpf_bw=0.005):
    """-> (loop, plant, start state [5], goal, obstacle map)"""
    torch.manual_seed(seed)
    dt = 0.1
    obst_map = generate_obstacle_map(map_dim=(22, 22), obst_list=get_obst_preset(preset, obst_width=1.0), cell_size=0.1, map_type="direct")
    start, goal = torch.tensor([-2.9, -2.6, 0.6, 0.0, 0.0]), (2.6, 2.9, 0.0, 0.0, 0.0)
    cost = NavigationCost(goal, (1.0, 1.0, 0.0, 0.0, 0.0), (20.0, 20.0, 0.0, 0.0, 0.0), None, obst_map=obst_map, w_obs=w_obs)
    model = SkidSteerRobot(delta_t=dt, wheel_radius=BELIEF, uncertain_params=("wheel_radius",), min_wheel_speed=-3.0, max_wheel_speed=3.0)
    plant = SkidSteerRobot(delta_t=dt, wheel_radius=TRUE_RADIUS, min_wheel_speed=-3.0, max_wheel_speed=3.0)
    ctrl = AMPPI(model.observation_space, model.action_space, horizon, samples, lambda_=5.0, a_cov=torch.eye(2), inst_cost_fn=cost.inst_cost,
                 term_cost_fn=cost.term_cost, params_sampling=sampling, init_actions=1.5 * torch.ones(horizon, 2), seed=seed)
    ctrl.return_rollouts = False
    x0 = BELIEF + 0.01 * torch.randn(mpf_particles, 1)
    # the observed speeds are v = pi (r + l) wheel_radius and omega = 2 pi (r - l) wheel_radius / axial_distance: at wheel speeds of
    # +-3 rot/s the log-likelihood's curvature in wheel_radius reaches ((6 pi)^2 + (12 pi / 0.475)^2) / obs_std^2 = 2.7e6, so plain SGD
    # is stable below lr = 7e-7.  A FIXED bandwidth (as examples/skid_steer_example.py has): one update pulls the particles together, and
    # Silverman's rule (mpf_bw=None) then gives a bandwidth of 1e-6 whose repulsion term throws them apart - the reference's filter does so too
    mpf = MPF(init_particles=x0, likelihood=GaussianLikelihood(initial_obs=start, obs_std=0.05, model=model, log_space=False),
              optimizer_class=torch.optim.SGD, lr=2e-7, bw=mpf_bw, bw_scale=1.0)
    return DualAMPPI(ctrl, model, mpf, mpf_bw=mpf_bw, mpf_steps=20, fused=fused, seed=seed), plant, start, goal, obst_map


def main(argv=None):
    """-> the plant's states [ticks + 1, 5]"""
    ap = argparse.ArgumentParser()
    ap.add_argument("--horizon", type=int, default=20)
    ap.add_argument("--ticks", type=int, default=100)
    ap.add_argument("--samples", type=int, default=1024)
    ap.add_argument("--mpf-particles", type=int, default=64)
    ap.add_argument("--preset", default="grid_6x6")
    ap.add_argument("--w-obs", type=float, default=20.0)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--unfused", action="store_true", help="the hand composition: parameter rows through the host every tick")
    ap.add_argument("--verbose", action="store_true")
    a = ap.parse_args(argv)
    loop, plant, start, goal, obst_map = scenario(a.samples, a.horizon, a.mpf_particles, a.preset, a.w_obs, a.seed, not a.unfused)
    state, states, hits = start.reshape(1, -1), [start.clone()], 0
    for t in range(a.ticks):
        action, state, _ = loop.tick(state, lambda x, u: plant.step(x.reshape(1, -1), u.reshape(1, -1)))
        states.append(state.reshape(-1).clone())
        hits += int(obst_map.get_collisions(state.reshape(1, -1)[:, 0:2]).item())
        if a.verbose:
            print("tick %3d  action (%+.2f, %+.2f)  state (%+.2f, %+.2f, %+.2f)" % ((t,) + tuple(action.tolist()) + tuple(state.reshape(-1)[:3].tolist())))
    states = torch.stack(states)
    d0, d1 = (float((x[:2] - torch.tensor(goal[:2])).norm()) for x in (states[0], states[-1]))
    print("%d ticks: distance to the goal %.2f -> %.2f m, %d steps on occupied cells, wheel_radius estimate %.4f (belief %.4f, true %.4f)"
          % (a.ticks, d0, d1, hits, float(loop.dyn_particles.mean()), BELIEF, TRUE_RADIUS))
    return states


if __name__ == "__main__":
    main()
