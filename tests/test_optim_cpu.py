"""The device optimisers on the CPU side (dust_amd/optim.py, include/dust_amd.h dust_optim_config): what each torch.optim class and
its options map to, what is refused, and that SVMPC / MPF hand every option to the device instead of dropping it.  No GPU."""
import ctypes as C
import os
import subprocess
import tempfile

import pytest
import torch

from conftest import ROOT


def _oc(cls, **kw):
    from dust_amd.optim import optimizer_config

    return optimizer_config(cls, kw)


def test_sgd_options():
    o = _oc(torch.optim.SGD, lr=2.0, momentum=0.9, nesterov=True, weight_decay=0.01, maximize=True)
    assert (o["kind"], o["lr"], o["momentum"], o["dampening"], o["weight_decay"]) == ("SGD", 2.0, 0.9, 0.0, 0.01)
    assert o["nesterov"] and o["maximize"] and not o["amsgrad"]
    d = _oc(torch.optim.SGD)
    assert (d["lr"], d["momentum"], d["weight_decay"], d["nesterov"], d["maximize"]) == (1e-3, 0.0, 0.0, False, False)


def test_adam_and_adamw_defaults():
    a = _oc(torch.optim.Adam)
    assert (a["kind"], a["lr"], a["beta1"], a["beta2"], a["eps"], a["weight_decay"]) == ("Adam", 1e-3, 0.9, 0.999, 1e-8, 0.0)
    assert not a["decoupled_weight_decay"] and not a["amsgrad"]
    w = _oc(torch.optim.AdamW)
    assert w["kind"] == "Adam" and w["weight_decay"] == 0.01 and w["decoupled_weight_decay"]  # AdamW's default decay is 0.01, decoupled
    w2 = _oc(torch.optim.AdamW, lr=0.5, betas=(0.8, 0.99), weight_decay=0.1, amsgrad=True, maximize=True)
    assert (w2["lr"], w2["beta1"], w2["beta2"], w2["weight_decay"]) == (0.5, 0.8, 0.99, 0.1)
    assert w2["amsgrad"] and w2["maximize"] and w2["decoupled_weight_decay"]
    assert _oc(torch.optim.Adam, decoupled_weight_decay=True, weight_decay=0.2)["decoupled_weight_decay"]


def test_rmsprop_and_adagrad_defaults():
    r = _oc(torch.optim.RMSprop)
    assert (r["kind"], r["lr"], r["alpha"], r["eps"], r["momentum"], r["weight_decay"], r["centered"]) == ("RMSprop", 1e-2, 0.99, 1e-8, 0.0, 0.0, False)
    r2 = _oc(torch.optim.RMSprop, lr=0.1, alpha=0.9, momentum=0.5, centered=True, weight_decay=0.01, maximize=True)
    assert (r2["alpha"], r2["momentum"], r2["weight_decay"]) == (0.9, 0.5, 0.01) and r2["centered"] and r2["maximize"]
    g = _oc(torch.optim.Adagrad)
    assert (g["kind"], g["lr"], g["lr_decay"], g["eps"], g["initial_accumulator_value"], g["weight_decay"]) == ("Adagrad", 1e-2, 0.0, 1e-10, 0.0, 0.0)
    g2 = _oc(torch.optim.Adagrad, lr=0.5, lr_decay=0.1, initial_accumulator_value=0.2, eps=1e-6)
    assert (g2["lr_decay"], g2["initial_accumulator_value"], g2["eps"]) == (0.1, 0.2, 1e-6)


@pytest.mark.parametrize("cls", [torch.optim.Adamax, torch.optim.NAdam, torch.optim.RAdam, torch.optim.ASGD, torch.optim.Rprop,
                                 torch.optim.LBFGS, torch.optim.SparseAdam, torch.optim.Adadelta])
def test_other_classes_are_refused(cls):
    with pytest.raises(NotImplementedError, match=cls.__name__):
        _oc(cls)


@pytest.mark.parametrize("cls,kw,word", [
    (torch.optim.Adam, dict(capturable=True), "capturable"),
    (torch.optim.RMSprop, dict(differentiable=True), "differentiable"),
    (torch.optim.SGD, dict(foreach=True), "foreach"),
    (torch.optim.Adam, dict(fused=True), "fused"),
    (torch.optim.Adam, dict(lr=torch.tensor(0.01)), "tensor lr"),
    (torch.optim.SGD, dict(params=[{"params": []}]), "param group"),
])
def test_flags_are_refused(cls, kw, word):
    with pytest.raises(NotImplementedError, match=word):
        _oc(cls, **kw)


def test_invalid_values_raise_as_torch_does():
    with pytest.raises(ValueError):
        _oc(torch.optim.SGD, lr=1.0, nesterov=True)  # nesterov without momentum
    with pytest.raises(ValueError):
        _oc(torch.optim.Adam, betas=(1.5, 0.9))


def test_struct_round_trip():
    from dust_amd import _lib as L
    from dust_amd.optim import from_struct, is_plain, to_struct

    for cls, kw in [(torch.optim.SGD, dict(lr=2.0, momentum=0.9, nesterov=True, maximize=True)),
                    (torch.optim.AdamW, dict(amsgrad=True)), (torch.optim.RMSprop, dict(centered=True, momentum=0.3)),
                    (torch.optim.Adagrad, dict(lr_decay=0.1, initial_accumulator_value=0.5))]:
        o = _oc(cls, **kw)
        s = to_struct(o)
        assert from_struct(s) == o
        assert not is_plain(o)
    s = to_struct(_oc(torch.optim.AdamW, amsgrad=True))
    assert s.kind == L.OPT_ADAM and s.flags == L.OPTF_AMSGRAD | L.OPTF_DECOUPLED_WD
    assert is_plain(_oc(torch.optim.SGD, lr=2.0, momentum=0.0, dampening=0.0, weight_decay=0.0))
    assert is_plain(_oc(torch.optim.Adam, lr=0.5, weight_decay=0.0, amsgrad=False))


def test_optim_struct_matches_header():
    """sizeof(dust_optim_config) of a C compile against include/dust_amd.h equals its ctypes mirror."""
    from dust_amd import _lib

    src = '#include "dust_amd.h"\n#include <stdio.h>\n#include <stddef.h>\nint main(){printf("%zu %zu %zu", sizeof(dust_optim_config), ' \
          'offsetof(dust_optim_config, lr), offsetof(dust_optim_config, initial_accumulator_value));return 0;}\n'
    with tempfile.TemporaryDirectory() as d:
        p = os.path.join(d, "p.c")
        open(p, "w").write(src)
        subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), p, "-o", os.path.join(d, "p")], check=True)
        out = subprocess.run([os.path.join(d, "p")], check=True, capture_output=True, text=True).stdout.split()
    S = _lib.OptimConfig
    assert [int(v) for v in out] == [C.sizeof(S), S.lr.offset, S.initial_accumulator_value.offset]


def _svmpc(optimizer_class, **opt_args):
    from dust_amd.controllers import MultiDISCO
    from dust_amd.inference import SVMPC, ExponentiatedUtility, get_gmm
    from dust_amd.kernels import RBFKernel
    from dust_amd.models import PendulumModel

    N, H, S = 8, 5, 16
    model = PendulumModel()
    ctrl = MultiDISCO(model.observation_space, model.action_space, H, N, S, temperature=1.0, a_cov=4.0 * torch.eye(1),
                      inst_cost_fn=lambda s, controls=None, n_pol=1, debug=None: s[..., 0] ** 2,
                      term_cost_fn=lambda s, n_pol=1, debug=None: s[..., 0] ** 2, params_sampling=None)
    prior = get_gmm(torch.zeros(N, H, 1), torch.ones(N), 4.0 * torch.eye(1))
    lik = ExponentiatedUtility(alpha=1.0, n_samples=S, controller=ctrl, model=model)
    sv = SVMPC(init_particles=torch.zeros(N, H, 1), prior=prior, likelihood=lik, kernel=RBFKernel(), n_particles=N, bw_scale=1.0,
               n_steps=1, optimizer_class=optimizer_class, **opt_args)
    return sv, ctrl


def test_svmpc_momentum_reaches_the_device_config():
    """SVMPC(optimizer_class=SGD, lr=2.0, momentum=0.9) used to build a plain-SGD device config and drop the momentum silently."""
    sv, ctrl = _svmpc(torch.optim.SGD, lr=2.0, momentum=0.9)
    oc = ctrl._svmpc_cfg["optim"]
    assert oc["kind"] == "SGD" and oc["momentum"] == 0.9 and oc["lr"] == 2.0
    from dust_amd.optim import is_plain

    assert not is_plain(oc)
    sv2, ctrl2 = _svmpc(torch.optim.Adam, lr=0.1, amsgrad=True, weight_decay=0.01)
    assert ctrl2._svmpc_cfg["optim"]["amsgrad"] and ctrl2._svmpc_cfg["optim"]["weight_decay"] == 0.01


def test_svmpc_refuses_what_the_device_lacks():
    with pytest.raises(NotImplementedError, match="NAdam"):
        _svmpc(torch.optim.NAdam, lr=0.1)
    with pytest.raises(NotImplementedError, match="foreach"):
        _svmpc(torch.optim.RMSprop, lr=0.1, foreach=True)


def test_lr_scheduler_and_param_groups_are_refused():
    from dust_amd.optim import check_optimizer

    sv, _ = _svmpc(torch.optim.SGD, lr=2.0, momentum=0.9)
    check_optimizer(sv.optimizer, sv._opt_group)  # as constructed: fine
    torch.optim.lr_scheduler.StepLR(sv.optimizer, step_size=1)
    with pytest.raises(NotImplementedError, match="scheduler"):
        check_optimizer(sv.optimizer, sv._opt_group)
    sv, _ = _svmpc(torch.optim.Adagrad, lr=0.5)
    sv.optimizer.add_param_group({"params": [torch.zeros(1, requires_grad=True)]})
    with pytest.raises(NotImplementedError, match="param group"):
        check_optimizer(sv.optimizer, sv._opt_group)


@pytest.mark.parametrize("key,value", [("lr", 0.1), ("momentum", 0.5), ("nesterov", True), ("weight_decay", 0.01), ("maximize", True)])
def test_option_edits_after_construction_are_refused(key, value):
    """Editing any option of sv.optimizer's group after construction would not reach the device: refused, not dropped."""
    from dust_amd.optim import check_optimizer

    sv, _ = _svmpc(torch.optim.SGD, lr=2.0, momentum=0.9)
    sv.optimizer.param_groups[0][key] = value
    with pytest.raises(NotImplementedError, match=key):
        check_optimizer(sv.optimizer, sv._opt_group)
