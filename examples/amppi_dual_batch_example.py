#!/usr/bin/env python3
"""B episodes of the dual loop at once on the MI355X backend: `BatchDualAMPPI` runs B pendulums, each with its OWN true mass and length,
on one `BatchAMPPI` (the control side: B ticks in one launch) and B copies of one `MPF` (the dynamics side: B filter updates in one
launch) - the batch counterpart of examples/amppi_dual_example.py.  The reference evaluates the dual controller over many episodes and
gives each a deep copy of the controller and of the filter (dust/utils/simulations.py:62,78); here a control period of all of them is
one C call (dust_amppi_dual_batch_tick) whose number of kernel launches does not depend on B.  The plants are host `PendulumModel`s.

    python examples/amppi_dual_batch_example.py --envs 8 --ticks 100
"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from dust_amd.controllers import AMPPI, BatchAMPPI, BatchDualAMPPI, DualAMPPI  # noqa: E402
from dust_amd.costs import PendulumQuadCos  # noqa: E402
from dust_amd.inference import MPF, GaussianLikelihood  # noqa: E402
from dust_amd.models import PendulumModel  # noqa: E402

LAMBDA, A_COV, LR, OBS_STD, INIT_BW = 100.0, 4.0, 1e-3, 0.1, 0.1


def truths(n_envs, seed=0):
    """-> (true lengths [B], true masses [B], start states [B, 2], the filters' first particles [B, Mp, 2] are drawn by `particles`)"""
    g = torch.Generator().manual_seed(1000 + seed)
    length = 0.8 + 0.5 * torch.rand(n_envs, generator=g)
    mass = 0.8 + 0.5 * torch.rand(n_envs, generator=g)
    start = torch.tensor([3.0, 0.0]) + 0.2 * torch.randn(n_envs, 2, generator=g)
    return length, mass, start


def particles(n_envs, mpf_particles, seed=0):
    """every environment's belief over (length, mass): [B, Mp, 2] round (1, 1)"""
    g = torch.Generator().manual_seed(2000 + seed)
    return 1.0 + 0.1 * torch.randn(n_envs, mpf_particles, 2, generator=g)


def _filter(model, x0, start, mpf_bw):
    return MPF(init_particles=x0, likelihood=GaussianLikelihood(initial_obs=start, obs_std=OBS_STD, model=model, log_space=False),
               optimizer_class=torch.optim.SGD, lr=LR, bw=INIT_BW, bw_scale=1.0)


def _controller_args(model, horizon, samples, sampling, seed):
    cost = PendulumQuadCos()
    return (model.observation_space, model.action_space, horizon, samples), dict(
        lambda_=LAMBDA, a_cov=A_COV * torch.eye(1), inst_cost_fn=cost.inst_cost, term_cost_fn=cost.term_cost, params_sampling=sampling, seed=seed)


def scenario(n_envs=8, samples=1024, horizon=20, mpf_particles=64, seed=0, sampling="extended", mpf_bw=None, mpf_steps=20):
    """-> (loop, plant(states [B, 2], actions [B, 1]) -> new states, start states [B, 2], (true lengths, true masses))"""
    length, mass, start = truths(n_envs, seed)
    x0 = particles(n_envs, mpf_particles, seed)
    model = PendulumModel(uncertain_params=("length", "mass"))
    args, kw = _controller_args(model, horizon, samples, sampling, seed)
    ctrl = BatchAMPPI(n_envs, *args, **kw)
    ctrl.return_rollouts = False
    mpf = _filter(model, x0[0], start[0], mpf_bw)
    loop = BatchDualAMPPI(ctrl, model, mpf, mpf_bw=mpf_bw, mpf_steps=mpf_steps, seed=seed, init_particles=x0)
    plants = [PendulumModel(length=float(length[b]), mass=float(mass[b])) for b in range(n_envs)]

    def plant(states, actions):
        states, actions = torch.as_tensor(states, dtype=torch.float), torch.as_tensor(actions, dtype=torch.float)
        return torch.stack([plants[b].step(states[b].reshape(1, -1), actions[b].reshape(1, -1)).reshape(-1) for b in range(n_envs)])

    return loop, plant, start, (length, mass)


def lone(b, n_envs=8, samples=1024, horizon=20, mpf_particles=64, seed=0, sampling="extended", mpf_bw=None, mpf_steps=20):
    """Environment b of `scenario` as an object of its own: -> (DualAMPPI(fused=True), plant(state, action) -> new state, start state [2]).
    Its controller draws under the batch's seed + b, its prior keys start from seed + (b << 32): what the batch gives environment b."""
    length, mass, start = truths(n_envs, seed)
    x0 = particles(n_envs, mpf_particles, seed)
    model = PendulumModel(uncertain_params=("length", "mass"))
    args, kw = _controller_args(model, horizon, samples, sampling, seed + b)
    ctrl = AMPPI(*args, **kw)
    ctrl.return_rollouts = False
    loop = DualAMPPI(ctrl, model, _filter(model, x0[b], start[b], mpf_bw), mpf_bw=mpf_bw, mpf_steps=mpf_steps, fused=True, seed=seed + (b << 32))
    p = PendulumModel(length=float(length[b]), mass=float(mass[b]))
    return loop, (lambda x, u: p.step(x.reshape(1, -1), u.reshape(1, -1))), start[b]


def main(argv=None):
    """-> the plants' states [ticks + 1, B, 2]"""
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=8)
    ap.add_argument("--horizon", type=int, default=20)
    ap.add_argument("--ticks", type=int, default=100)
    ap.add_argument("--samples", type=int, default=1024)
    ap.add_argument("--mpf-particles", type=int, default=64)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--verbose", action="store_true")
    a = ap.parse_args(argv)
    loop, plant, start, (length, mass) = scenario(a.envs, a.samples, a.horizon, a.mpf_particles, a.seed)
    states, trace = start.clone(), [start.clone()]
    for t in range(a.ticks):
        actions, states, _ = loop.tick(states, plant)
        trace.append(states.clone())
        if a.verbose:
            print("tick %3d  torque %s" % (t, " ".join("%+.2f" % float(u) for u in actions.reshape(-1))))
    x = loop.dyn_particles.mean(1)
    err0 = float(((1.0 - length) ** 2 + (1.0 - mass) ** 2).sqrt().mean())
    err1 = float(((x[:, 0] - length) ** 2 + (x[:, 1] - mass) ** 2).sqrt().mean())
    print("%d ticks of %d pendulums: mean |angle| %.2f -> %.2f rad, mean parameter error %.3f -> %.3f"
          % (a.ticks, a.envs, float(trace[0][:, 0].abs().mean()), float(trace[-1][:, 0].abs().mean()), err0, err1))
    return torch.stack(trace)


if __name__ == "__main__":
    main()
