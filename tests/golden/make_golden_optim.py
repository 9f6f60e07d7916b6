#!/usr/bin/env python3
"""Golden vectors of the reference's SVMPC / MPF run with optimisers other than plain SGD / Adam (svgd.py:109-125 takes any
torch.optim class with its **opt_args).

TEST INFRASTRUCTURE.  Run from the repo root:  python tests/golden/make_golden_optim.py
Needs the reference (build container only); writes tests/golden/*.npz (small, committed).

The same recording machinery as make_golden.py (run_svmpc, run_mpf): the reference's own SVMPC / MPF are constructed by those
functions; here only the optimiser class and its options are handed to the constructor instead of the SGD / Adam those
functions name.  Each fixture also stores `opt_class` and `opt_args` (JSON) so the test builds the same optimiser.

Adagrad: torch's Adagrad creates its state in __init__ only, so once SVMPC.roll (svmpc.py:158) has swapped a new tensor into the
param group the reference's next step() raises KeyError('sum').  part_k1_adagrad is therefore ONE tick (no roll inside the
recorded chain); the device restarts `sum` at initial_accumulator_value at a roll instead (include/dust_amd.h dust_set_optimizer).
"""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import make_golden as mg  # noqa: E402  (installs the shim, imports the reference)

import numpy as np  # noqa: E402
import torch  # noqa: E402


def _with_optimizer(runner, ctor_name, tag, cls, opt, **kw):
    """run `runner` (mg.run_svmpc / mg.run_mpf) with the reference class `ctor_name` constructed with optimizer_class=cls, **opt"""
    orig = getattr(mg, ctor_name)

    def ctor(**a):
        a.update(optimizer_class=cls, **opt)
        return orig(**a)

    setattr(mg, ctor_name, ctor)
    try:
        runner(tag, **kw)
    finally:
        setattr(mg, ctor_name, orig)
    path = os.path.join(mg.OUT, tag + ".npz")
    g = dict(np.load(path, allow_pickle=False))
    g.update(opt_class=cls.__name__, opt_args=json.dumps(opt), lr=float(opt["lr"]))
    np.savez_compressed(path, **g)
    print("  with", cls.__name__, opt, "%.0f KB" % (os.path.getsize(path) / 1024))


if __name__ == "__main__":
    S, M = mg.run_svmpc, mg.run_mpf
    _with_optimizer(S, "SVMPC", "pend_k1_sgdmom_nesterov", torch.optim.SGD, dict(lr=0.5, momentum=0.9, nesterov=True),
                    model_kind="pendulum", N=16, H=10, S=8, M=1, kernel_kind="K1", n_iters=3, n_ticks=3, seed=40)
    _with_optimizer(S, "SVMPC", "pend_k1_rmsprop_centered_mom", torch.optim.RMSprop,
                    dict(lr=0.05, alpha=0.9, momentum=0.5, centered=True, weight_decay=0.01),
                    model_kind="pendulum", N=16, H=10, S=8, M=1, kernel_kind="K1", n_iters=3, n_ticks=3, seed=41)
    _with_optimizer(S, "SVMPC", "part_k1_adagrad", torch.optim.Adagrad, dict(lr=0.5, lr_decay=0.1, initial_accumulator_value=0.2),
                    model_kind="particle", N=8, H=12, S=8, M=4, kernel_kind="K1", weighted_prior=True, n_iters=3, n_ticks=1, seed=42,
                    params_kind="logmass_gmm")
    _with_optimizer(S, "SVMPC", "pend_k1_adamw_amsgrad", torch.optim.AdamW, dict(lr=0.1, amsgrad=True, maximize=False),
                    model_kind="pendulum", N=16, H=10, S=8, M=1, kernel_kind="K1", n_iters=3, n_ticks=3, seed=43)
    _with_optimizer(S, "SVMPC", "pend_k2_rmsprop", torch.optim.RMSprop, dict(lr=0.05),
                    model_kind="pendulum", N=16, H=10, S=8, M=1, kernel_kind="K2", n_iters=3, n_ticks=2, seed=44)
    _with_optimizer(M, "MPF", "mpf_pend_rmsprop", torch.optim.RMSprop, dict(lr=0.002, momentum=0.3),
                    model_kind="pendulum", Mp=10, n_steps=6, log_space=False, bw=0.08)
    _with_optimizer(M, "MPF", "mpf_part_log_adagrad", torch.optim.Adagrad, dict(lr=0.02, lr_decay=0.05, initial_accumulator_value=0.1),
                    model_kind="particle", Mp=12, n_steps=12, log_space=True, bw=0.5)
