#!/usr/bin/env python3
"""B episodes of the DuSt-MPC loop with the plants on the device: the B pendulums of examples/svmpc_dual_batch_example.py, each with its
OWN true length and mass, but stepped by the library (`BatchDualSVMPC.run_episodes`, dust_svmpc_dual_batch_episode) and not by host
`PendulumModel`s.  A control period is the filters' update for (a_{t-1}, x_t), the B ticks whose workgroups draw their dynamics samples
from their own environment's refreshed filter prior, and the plant's step under the environment's true parameters - all queued on one
stream; nothing crosses the bus between the periods of one `run_episodes` call.  An episode is run in pieces of `--piece` periods: the
pieces chain through the pending pair (the last action and state), so any split computes the same episode.

    python examples/svmpc_dual_episode_example.py --envs 8 --ticks 96 --piece 32
"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from svmpc_dual_batch_example import scenario  # noqa: E402

from dust_amd.costs import PendulumQuadCos  # noqa: E402

TINY = dict(n_envs=3, ticks=4, piece=2, particles=2, samples=8, params=2, horizon=4, mpf_particles=8, mpf_steps=2)


def run(n_envs=8, ticks=96, piece=32, particles=3, samples=128, params=8, horizon=30, mpf_particles=256, mpf_steps=20, seed=0, quiet=False):
    """-> (average cost per environment [B], the filters' mean estimates [B, 2], the true (length, mass) [B, 2])"""
    loop, _, start, (length, mass) = scenario(n_envs, particles, samples, params, horizon, mpf_particles, seed, mpf_steps=mpf_steps)
    true = torch.stack((length, mass), 1)  # the columns of the filters' particles: (length, mass)
    cost = PendulumQuadCos()
    states, total, done = start.clone(), torch.zeros(n_envs), 0
    while done < ticks:
        T = min(piece, ticks - done)
        xs, acts, _, _ = loop.run_episodes(states, T, plant_params=true)  # ONE call per episode piece
        before = torch.cat((states[None], xs[:-1]))  # the state every period's action was chosen in
        total += cost.inst_cost(before.reshape(T * n_envs, 2), acts.reshape(T * n_envs, 1)).reshape(T, n_envs).sum(0)
        states, done = xs[-1], done + T
    avg = total / ticks
    est = loop.dyn_particles.mean(1)  # (folds the pending pair in first)
    if not quiet:
        print("%d periods of %d pendulums in pieces of %d: final mean |angle| %.2f rad" % (ticks, n_envs, piece, float(states[:, 0].abs().mean())))
        for b in range(n_envs):
            print("  env %2d  average cost %9.3f   length %.3f (true %.3f)   mass %.3f (true %.3f)"
                  % (b, float(avg[b]), float(est[b, 0]), float(length[b]), float(est[b, 1]), float(mass[b])))
    return avg, est, true


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=8)
    ap.add_argument("--ticks", type=int, default=96)
    ap.add_argument("--piece", type=int, default=32)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--tiny", action="store_true", help="the size the test suite runs")
    a = ap.parse_args(argv)
    if a.tiny:
        return run(seed=a.seed, **TINY)
    return run(a.envs, a.ticks, a.piece, seed=a.seed)


if __name__ == "__main__":
    main()
