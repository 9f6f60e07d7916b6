"""Device-side helpers (TEST INFRASTRUCTURE) shared by tests/test_gpu_disco_batch.py and tests/test_gpu_disco_episode.py: the batch of a case
of tests/disco_cases.py, its getters, and a `BatchDISCO` beside lone `MultiDISCO` objects.  The library is imported inside the functions."""
import numpy as np
import torch

import disco_cases as dc

GETTERS = ("A_MAT", "A_SEQ", "A_MIX", "COSTS", "OMEGA")
COST_TOL, EXP_TOL = 2e-5, 5e-4  # tests/test_gpu_svmpc_batch.py, item 2


def _L():
    from dust_amd import _lib

    return _lib


def _records(b, actions=False):
    L = _L()
    return {n: b.get(getattr(L, "DCB_" + n)) for n in GETTERS + (("ACTIONS",) if actions else ())}


def _same(x, y, rows=slice(None)):
    for n in x:
        assert np.array_equal(x[n][rows], y[n][rows]), n


def _grid(case):
    if case["family"] == "particle":
        from oracle import grid_4x4_map

        return grid_4x4_map()
    return dc.nav_map() if case["nav"] else None


def _proto(case, **kw):
    from dust_amd import Context

    c = Context(grid=_grid(case), **dc.context_kwargs(case, **kw))
    if case["sigma"]:
        w, scale = dc.sigma_weights(case)
        c.set_param_weights(w.astype(np.float32))
        c.set_sigma_scale(float(scale))
    return c


def _batch(case, inp, envs=None):
    """a batch whose slot k holds environment envs[k] of the case (default: all of them, in order)"""
    L = _L()
    envs = list(range(case["B"])) if envs is None else list(envs)
    c = _proto(case)
    b = c.disco_batch(len(envs), seeds=[inp["seeds"][e] for e in envs])
    c.close()
    b.set(L.DCB_A_MAT, inp["a_mat"][envs])
    b.set(L.DCB_A_SEQ, inp["a_seq"][envs])
    return b


def _sub(inp, envs, k):
    return None if inp[k] is None else np.ascontiguousarray(inp[k][list(envs)])


def _pair(n_envs, seeds, N=3, S=16, H=6, M=2, ctrl_penalty=0.7):
    from dust_amd.controllers import BatchDISCO, MultiDISCO
    from dust_amd.costs import PendulumQuadCos
    from dust_amd.models import PendulumModel

    model, cost = PendulumModel(uncertain_params=("length", "mass")), PendulumQuadCos()
    kw = dict(temperature=20.0, ctrl_penalty=ctrl_penalty, a_cov=4.0 * torch.eye(1), inst_cost_fn=cost.inst_cost, term_cost_fn=cost.term_cost,
              params_sampling=True, params_samples=M)
    batch = BatchDISCO(n_envs, model.observation_space, model.action_space, H, N, S, seeds=seeds, **kw)
    lone = [MultiDISCO(model.observation_space, model.action_space, H, N, S, seed=s, **kw) for s in seeds]
    return model, batch, lone
