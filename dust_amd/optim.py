"""torch.optim classes on the device: `optimizer_config(optimizer_class, opt_args)` maps a class and its options to the device's optimiser
(include/dust_amd.h dust_optim_config) or raises for what the HIP kernels do not implement.  Pure Python: it needs no GPU.

SVGD takes an ordinary optimiser step on the particles with grad = -phi (svgd.py:109-125, svmpc.py:87-95, mpf.py:59-62); the device
follows the installed torch's single-tensor CPU functions (`_single_tensor_sgd / _adam / _rmsprop / _adagrad`) for:

    SGD      lr, momentum, dampening, weight_decay, nesterov, maximize
    Adam     lr, betas, eps, weight_decay, amsgrad, maximize, decoupled_weight_decay
    AdamW    the same (decoupled weight decay, default weight_decay 0.01)
    RMSprop  lr, alpha, eps, weight_decay, momentum, centered, maximize
    Adagrad  lr, lr_decay, weight_decay, initial_accumulator_value, eps, maximize
"""
import torch

from . import _lib as L

# per class: the options the device honours (every other constructor option must keep its torch default)
_HONOURED = {
    "SGD": ("lr", "momentum", "dampening", "weight_decay", "nesterov", "maximize"),
    "Adam": ("lr", "betas", "eps", "weight_decay", "amsgrad", "maximize", "decoupled_weight_decay"),
    "RMSprop": ("lr", "alpha", "eps", "weight_decay", "momentum", "centered", "maximize"),
    "Adagrad": ("lr", "lr_decay", "weight_decay", "initial_accumulator_value", "eps", "maximize"),
}
_KIND = {"SGD": L.OPT_SGD, "Adam": L.OPT_ADAM, "RMSprop": L.OPT_RMSPROP, "Adagrad": L.OPT_ADAGRAD}
_FIELDS = ("lr", "beta1", "beta2", "eps", "weight_decay", "momentum", "dampening", "alpha", "lr_decay", "initial_accumulator_value")


def _family(optimizer_class):
    if optimizer_class is torch.optim.SGD:
        return "SGD"
    if optimizer_class is torch.optim.Adam or optimizer_class is torch.optim.AdamW:
        return "Adam"
    if optimizer_class is torch.optim.RMSprop:
        return "RMSprop"
    if optimizer_class is torch.optim.Adagrad:
        return "Adagrad"
    raise NotImplementedError("optimizer %r has no HIP kernel: the device implements torch.optim.SGD, Adam, AdamW, RMSprop and Adagrad"
                              % (getattr(optimizer_class, "__name__", optimizer_class),))


def optimizer_config(optimizer_class, opt_args):
    """The device optimiser for `optimizer_class(params, **opt_args)`: a dict with `kind` (SGD / Adam / RMSprop / Adagrad; AdamW is Adam
    with decoupled weight decay), the scalars of dust_optim_config with torch's defaults filled in, and the flags (`maximize`,
    `nesterov`, `amsgrad`, `decoupled_weight_decay`, `centered`).  Raises NotImplementedError for a class or an option the kernels do
    not implement, and torch's own ValueError / TypeError for invalid values."""
    fam = _family(optimizer_class)
    opt_args = dict(opt_args)
    for k in ("params", "param_groups"):
        if k in opt_args:
            raise NotImplementedError("more than one param group: the device optimises one particle tensor")
    lr = opt_args.get("lr", None)
    if isinstance(lr, torch.Tensor):
        raise NotImplementedError("a tensor lr is not implemented on the device (pass a Python float)")
    # torch's constructor checks the values and fills in its defaults (one placeholder parameter, never stepped)
    d = dict(optimizer_class([torch.zeros(1, requires_grad=True)], **opt_args).defaults)
    for k in ("capturable", "differentiable"):
        if d.get(k):
            raise NotImplementedError("%s=True is not implemented on the device" % k)
    if d.get("fused"):
        raise NotImplementedError("fused=True is not implemented on the device")
    if d.get("foreach"):
        raise NotImplementedError("foreach=True is not implemented on the device (the single-tensor step is what it follows)")
    if isinstance(d.get("lr"), torch.Tensor):
        raise NotImplementedError("a tensor lr is not implemented on the device (pass a Python float)")
    for k in ("capturable", "differentiable", "fused", "foreach"):
        d.pop(k, None)
    extra = sorted(set(d) - set(_HONOURED[fam]))
    if extra:
        raise NotImplementedError("optimiser options %s of %s are not implemented on the device" % (extra, optimizer_class.__name__))
    out = dict(kind=fam, lr=float(d["lr"]), beta1=0.0, beta2=0.0, eps=float(d.get("eps", 0.0)), weight_decay=float(d["weight_decay"]),
               momentum=float(d.get("momentum", 0.0)), dampening=float(d.get("dampening", 0.0)), alpha=float(d.get("alpha", 0.0)),
               lr_decay=float(d.get("lr_decay", 0.0)), initial_accumulator_value=float(d.get("initial_accumulator_value", 0.0)),
               maximize=bool(d["maximize"]), nesterov=bool(d.get("nesterov", False)), amsgrad=bool(d.get("amsgrad", False)),
               decoupled_weight_decay=bool(d.get("decoupled_weight_decay", False)), centered=bool(d.get("centered", False)))
    if fam == "Adam":
        b1, b2 = d["betas"]
        if isinstance(b1, torch.Tensor) or isinstance(b2, torch.Tensor):
            raise NotImplementedError("tensor betas are not implemented on the device (pass Python floats)")
        out["beta1"], out["beta2"] = float(b1), float(b2)
    return out


def is_plain(cfg):
    """True when `cfg` is what dust_config's own optimizer fields express (plain SGD, or Adam without options)."""
    if cfg["weight_decay"] != 0.0 or cfg["maximize"] or cfg["amsgrad"]:
        return False
    if cfg["kind"] == "SGD":
        return cfg["momentum"] == 0.0
    return cfg["kind"] == "Adam"


def to_struct(cfg):
    """dust_optim_config of a dict from optimizer_config."""
    o = L.OptimConfig()
    o.kind = _KIND[cfg["kind"]]
    o.flags = ((L.OPTF_MAXIMIZE if cfg["maximize"] else 0) | (L.OPTF_NESTEROV if cfg["nesterov"] else 0)
               | (L.OPTF_AMSGRAD if cfg["amsgrad"] else 0) | (L.OPTF_DECOUPLED_WD if cfg["decoupled_weight_decay"] else 0)
               | (L.OPTF_CENTERED if cfg["centered"] else 0))
    for f in _FIELDS:
        setattr(o, f, float(cfg[f]))
    return o


def from_struct(o):
    """The dict of optimizer_config for a dust_optim_config (dust_get_optimizer)."""
    kind = {v: k for k, v in _KIND.items()}[o.kind]
    out = dict(kind=kind, **{f: float(getattr(o, f)) for f in _FIELDS})
    out.update(maximize=bool(o.flags & L.OPTF_MAXIMIZE), nesterov=bool(o.flags & L.OPTF_NESTEROV), amsgrad=bool(o.flags & L.OPTF_AMSGRAD),
               decoupled_weight_decay=bool(o.flags & L.OPTF_DECOUPLED_WD), centered=bool(o.flags & L.OPTF_CENTERED))
    return out


def group_options(optimizer):
    """The options of the optimiser's (first) param group, without its parameters: what check_optimizer compares against."""
    return {k: v for k, v in optimizer.param_groups[0].items() if k != "params"}


def check_optimizer(optimizer, options):
    """Raises NotImplementedError when the torch optimiser object a controller exposes (`SVMPC.optimizer`) has been given what the
    device does not follow: a second param group, an LR scheduler, or any option changed after construction (`options`:
    group_options at construction - the device keeps those)."""
    groups = optimizer.param_groups
    if len(groups) != 1:
        raise NotImplementedError("more than one param group: the device optimises one particle tensor")
    g = groups[0]
    if "initial_lr" in g:
        raise NotImplementedError("LR schedulers are not implemented on the device (the step size is fixed at construction)")
    if len(g) != len(options) + 1 or any(k not in g or not _same(g[k], v) for k, v in options.items()):
        changed = sorted(k for k in set(g) - {"params"} if k not in options or not _same(g[k], options[k]))
        raise NotImplementedError("optimiser options %s changed after construction; the device keeps the constructed ones" % changed)


def _same(a, b):
    if isinstance(a, torch.Tensor) or isinstance(b, torch.Tensor):
        return a is b
    return a == b

