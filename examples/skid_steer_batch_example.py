#!/usr/bin/env python3
"""B skid-steer robots round ONE occupancy grid at once: one `BatchSVMPC` - B independent SVMPC controllers whose tick is ONE kernel launch
per control period - driven by `dust_amd.costs.NavigationCost` (a quadratic cost to the goal plus w_obs on every occupied cell of one of
`get_obst_preset`'s maps), against B host plants.  Every robot has its own start pose, its own true x_icr, its own particles, prior and
noise stream; the map, the model, the cost and the sizes are shared.  examples/skid_steer_example.py is the lone robot with a dynamics
filter; examples/svmpc_batch_example.py the batched pendulum.  Per period:

    a_seq, p = controller.tick(states, params_dist) -> first action of every sequence to its plant

    python examples/skid_steer_batch_example.py --envs 8 --ticks 100
    python examples/skid_steer_batch_example.py --tiny            (a few robots at a small size: what the tests run)
"""
import argparse
import math
import os
import sys
import time

import torch
import torch.distributions as dist

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from dust_amd.controllers import MultiDISCO  # noqa: E402
from dust_amd.costs import NavigationCost  # noqa: E402
from dust_amd.inference import BatchSVMPC, ExponentiatedUtility, get_gmm  # noqa: E402
from dust_amd.kernels import RBFKernel  # noqa: E402
from dust_amd.models import SkidSteerRobot  # noqa: E402
from dust_amd.utils.obstacle_map import generate_obstacle_map, get_obst_preset  # noqa: E402

TINY = dict(envs=3, ticks=3, particles=4, samples=8, params=2, horizon=6)


def main(argv=None):
    """-> the plants' states [ticks + 1, B, 5]"""
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=8, help="robots: environments of the batch")
    ap.add_argument("--ticks", type=int, default=100)
    ap.add_argument("--horizon", type=int, default=20)
    ap.add_argument("--particles", type=int, default=8, help="Stein particles per robot")
    ap.add_argument("--samples", type=int, default=32, help="action samples per particle")
    ap.add_argument("--params", type=int, default=4, help="dynamics samples per rollout")
    ap.add_argument("--preset", default="grid_6x6")
    ap.add_argument("--w-obs", type=float, default=20.0)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--tiny", action="store_true", help="%s" % ", ".join("%s %d" % kv for kv in TINY.items()))
    ap.add_argument("--verbose", action="store_true")
    a = ap.parse_args(argv)
    if a.tiny:
        for k, v in TINY.items():
            setattr(a, k, v)
    torch.manual_seed(a.seed)
    B, N, S, M, H, dt, sigma = a.envs, a.particles, a.samples, a.params, a.horizon, 0.1, 1.0
    obst_map = generate_obstacle_map(map_dim=(22, 22), obst_list=get_obst_preset(a.preset, obst_width=1.0), cell_size=0.1, map_type="direct")
    goal = (2.6, 2.9, 0.0, 0.0, 0.0)
    cost = NavigationCost(goal, (1.0, 1.0, 0.0, 0.0, 0.0), (20.0, 20.0, 0.0, 0.0, 0.0), (0.01, 0.01), obst_map=obst_map, w_obs=a.w_obs)
    # start poses along the lower left corner of the map, headings fanned towards the goal
    frac = torch.linspace(0.0, 1.0, B) if B > 1 else torch.zeros(1)
    states = torch.stack((-2.9 + 0.8 * frac, -2.6 - 0.3 * frac, 0.3 + 0.6 * frac, torch.zeros(B), torch.zeros(B)), 1)
    params_dist = dist.Independent(dist.Uniform(torch.tensor([0.15]), torch.tensor([0.35])), 1)  # x_icr: what the controller believes
    true_icr = params_dist.sample([B]).reshape(B)
    model = SkidSteerRobot(delta_t=dt, uncertain_params=("x_icr",), min_wheel_speed=-3.0, max_wheel_speed=3.0)
    plants = [SkidSteerRobot(delta_t=dt, x_icr=float(v), min_wheel_speed=-3.0, max_wheel_speed=3.0) for v in true_icr]
    ctrl = MultiDISCO(observation_space=model.observation_space, action_space=model.action_space, hz_len=H, n_policies=N, action_samples=S,
                      params_samples=M, temperature=5.0, a_cov=sigma ** 2 * torch.eye(2), inst_cost_fn=cost.inst_cost, term_cost_fn=cost.term_cost,
                      params_sampling=True, seed=a.seed)
    mu0 = 1.5 + 0.5 * torch.randn(N, H, 2)
    theta0 = mu0[None] + 0.3 * torch.randn(B, N, H, 2)  # every robot starts from its own particles
    ctrl.a_mat = mu0.clone()
    ctrl.return_rollouts = False
    controller = BatchSVMPC(B, theta0, get_gmm(mu0, torch.ones(N), sigma ** 2 * torch.eye(2)),
                            ExponentiatedUtility(alpha=0.2, n_samples=S, controller=ctrl, model=model), kernel=RBFKernel(), n_particles=N,
                            bw_scale=1.0, n_steps=1, optimizer_class=torch.optim.SGD, lr=0.5, seeds=[a.seed + b for b in range(B)])
    track, hits, t0 = [states.clone()], torch.zeros(B), time.perf_counter()
    for t in range(a.ticks):
        a_seq, _ = controller.tick(states, params_dist)  # ONE launch for the B ticks
        actions = a_seq[:, 0]  # [B, 2]
        states = torch.cat([plants[b].step(states[b:b + 1], actions[b:b + 1]) for b in range(B)], 0)
        track.append(states.clone())
        hits += obst_map.get_collisions(states[:, 0:2]).reshape(B)
        if a.verbose:
            print("tick %3d  " % t + "  ".join("(%+.2f, %+.2f)" % (float(x[0]), float(x[1])) for x in states))
    el = time.perf_counter() - t0
    track = torch.stack(track)
    g = torch.tensor(goal[:2])
    for b in range(B):
        d0, d1 = float((track[0, b, :2] - g).norm()), float((track[-1, b, :2] - g).norm())
        print("robot %2d  x_icr %.3f  distance to the goal %.2f -> %.2f m, %d steps on occupied cells" % (b, float(true_icr[b]), d0, d1, int(hits[b])))
    print("%d robots x %d periods round one %s map: %.1f environment-ticks/s incl. host plants" % (B, a.ticks, a.preset, B * a.ticks / el))
    assert math.isfinite(float(track.abs().max()))
    return track


if __name__ == "__main__":
    main()
