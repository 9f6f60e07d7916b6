#!/usr/bin/env python3
"""The posterior over the plant's parameters tightening while the controller runs - the data behind the reference's
`plot_dist_ridgeplot` (the `DynParticles` column of run_pendulum_simulation's frame) - out of the DEVICE episodes: B pendulums, each with
its own true (length, mass), run as the environments of one `BatchSVMPC` plus `BatchDualSVMPC` through
`run_pendulum_simulations(history=True)`.  The filters' particles of every period are recorded by the episode's own kernels
(`BatchDualSVMPC.set_history`, dust_svmpc_batch_set_history): no launch is added and the loop is never interrupted to read them.

At a handful of periods the script prints every filter's posterior mean and standard deviation beside the truth.  No plotting library
is needed: a ridge plot is a kernel density of each printed row's particles.

    python examples/pendulum_posterior_example.py --episodes 4 --steps 200 --warm-up 10
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from pendulum_dual_sim_example import TINY, run  # noqa: E402


def posterior_table(data, true, periods):
    """-> rows (period, episode, mean [P], std [P], truth [P]) of the filters after the pair of that period was folded in"""
    dyn = np.asarray(data["DynParticles"], np.float64)  # [B, steps, Mp, P]
    out = []
    for t in periods:
        for b in range(dyn.shape[0]):
            out.append((int(t), b, dyn[b, t].mean(0), dyn[b, t].std(0), np.asarray(true[b], np.float64)))
    return out


def report(episodes=4, steps=200, warm_up=10, seed=0, shown=5, quiet=False, **over):
    """-> (the dict of run_pendulum_simulations(history=True), the table of posterior_table)"""
    data, true = run(episodes, steps, warm_up, seed=seed, quiet=True, history=True, **over)
    periods = sorted({int(round(v)) for v in np.linspace(0, steps - 1, min(shown, steps))})
    table = posterior_table(data, true.numpy(), periods)
    if not quiet:
        pol = np.asarray(data["PolParticles"])  # [B, steps, N]: NaN while the episode warms up
        print("%d periods of %d pendulums, %d of them warm-up; posterior of (length, mass) per filter" % (steps, episodes, min(warm_up, steps)))
        for t, b, mean, std, truth in table:
            first = "warming up" if np.isnan(pol[b, t]).all() else "first actions " + " ".join("%6.2f" % v for v in pol[b, t])
            print("  period %4d  episode %2d  length %.3f +- %.3f (true %.3f)  mass %.3f +- %.3f (true %.3f)  %s"
                  % (t, b, mean[0], std[0], truth[0], mean[1], std[1], truth[1], first))
    return data, table


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--episodes", type=int, default=4)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warm-up", type=int, default=10)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--tiny", action="store_true", help="the size the test suite runs")
    a = ap.parse_args(argv)
    if a.tiny:
        return report(seed=a.seed, shown=3, **TINY)
    return report(a.episodes, a.steps, a.warm_up, seed=a.seed)


if __name__ == "__main__":
    main()
