"""The device optimisers (include/dust_amd.h dust_set_optimizer, dust_mpf_set_optimizer_ex; csrc/handoff.hpp opt_step) on the GPU:
step by step against torch.optim itself, the one-launch tick against the launch-per-iteration path, clones, and the plain SGD / Adam
of dust_config bit for bit."""
import os

import numpy as np
import pytest
import torch

from helpers import elemerr

pytestmark = pytest.mark.gpu

# (class, options): every option of the table in dust_amd/optim.py, with and without weight decay / maximize
CASES = [
    (torch.optim.SGD, dict(lr=0.5, momentum=0.9, nesterov=True)),
    (torch.optim.SGD, dict(lr=0.5, momentum=0.5, dampening=0.25, weight_decay=0.01, maximize=True)),
    (torch.optim.Adam, dict(lr=0.1, betas=(0.8, 0.99), amsgrad=True, weight_decay=0.01)),
    (torch.optim.AdamW, dict(lr=0.1, maximize=True)),
    (torch.optim.AdamW, dict(lr=0.1, amsgrad=True, weight_decay=0.05)),
    (torch.optim.RMSprop, dict(lr=0.05, alpha=0.9, momentum=0.5, centered=True)),
    (torch.optim.RMSprop, dict(lr=0.05, weight_decay=0.01, maximize=True)),
    (torch.optim.Adagrad, dict(lr=0.5, lr_decay=0.1, initial_accumulator_value=0.1)),
    (torch.optim.Adagrad, dict(lr=0.5, weight_decay=0.01, initial_accumulator_value=0.01, maximize=True)),
]
IDS = ["sgd_nesterov", "sgd_damp_wd_max", "adam_ams_wd", "adamw_max", "adamw_ams", "rmsprop_centered_mom", "rmsprop_wd_max",
       "adagrad_decay_init", "adagrad_wd_max"]
ENV_KEYS = ("DUST_NO_TICK2",)


def _state(model):
    return np.array([3.0, 0.0], np.float32) if model == "pendulum" else np.array([-9.0, -9.0, 0.0, 0.0], np.float32)


def _make(model, N, S, H, cls=None, opt=None, env=None, kernel="K1", seed=0, **kw):
    """a context created under the given development switches (the library reads them once, at dust_create)"""
    from dust_amd import Context
    from dust_amd.optim import optimizer_config

    da = 1 if model == "pendulum" else 2
    rng = np.random.default_rng(seed)
    mu = rng.standard_normal((N, H, da)).astype(np.float32)
    th = (mu + 2 * rng.standard_normal((N, H, da))).astype(np.float32)
    if model == "particle":
        from oracle import grid_4x4_map

        kw["grid"] = grid_4x4_map()
    sig = 2.0 if model == "pendulum" else 5.0
    if cls is not None:
        kw["optim"] = optimizer_config(cls, opt)
    saved = {k: os.environ.pop(k, None) for k in ENV_KEYS}
    os.environ.update(env or {})
    try:
        c = Context(model=model, N=N, S=S, M=1, H=H, kernel=kernel, sigma_a=sig, sigma_p=sig, seed=77,
                    **dict(dict(lr=2.0 if model == "pendulum" else 100.0), **kw))
    finally:
        for k in ENV_KEYS:
            os.environ.pop(k, None)
            if saved[k] is not None:
                os.environ[k] = saved[k]
    c.set_theta(th)
    c.set_prior(mu)
    c.set_a_mat(th)
    return c, rng


def _ulps(a, b, ref):
    """|a - b| in fp32 ulps of max(|b|, |ref|) (ref: the value before the step - a step that cancels keeps its size)"""
    scale = np.maximum(np.abs(b), np.abs(ref)).astype(np.float32)
    return float(np.max(np.abs(a.astype(np.float64) - b.astype(np.float64)) / np.spacing(np.maximum(scale, np.float32(1e-30)))))


# K1 for both models and every case; the K2 update sites (bandwidth.hpp) with the pendulum and RMSprop / AdamW
STEP_CASES = [(m, "K1", c, o) for m in ("pendulum", "particle") for c, o in CASES] + \
             [("pendulum", "K2", c, o) for c, o in CASES if c in (torch.optim.RMSprop, torch.optim.AdamW)]
STEP_IDS = ["%s-K1-%s" % (m, i) for m in ("pendulum", "particle") for i in IDS] + \
           ["pendulum-K2-%s" % i for (c, _), i in zip(CASES, IDS) if c in (torch.optim.RMSprop, torch.optim.AdamW)]


@pytest.mark.parametrize("model,kernel,cls,opt", STEP_CASES, ids=STEP_IDS)
def test_steps_follow_torch(model, kernel, cls, opt):
    """Launch-per-iteration path, one dust_svmpc_optimize step at a time: read phi and theta, apply the same step on the host with the real
    torch.optim class (grad = -phi of the device, state carried along and restarted where the device rolls: new parameter tensor), and
    hold theta to a few fp32 ulps element-wise.  phi is the same on both sides, so only the update arithmetic can differ."""
    N, S, H = 32, 64, 8
    c, rng = _make(model, N, S, H, cls, opt, env={"DUST_NO_TICK2": "1"}, kernel=kernel)
    da = 1 if model == "pendulum" else 2
    st = _state(model)
    for tick in range(2):
        p = torch.tensor(c.get_theta(), requires_grad=True)
        o = cls([p], **opt)
        for k in range(3):
            before = c.get_theta()
            eps = rng.standard_normal((1, S, N, H, da)).astype(np.float32)
            c.svmpc_optimize(st, 1, eps)
            phi, after = c.get_phi(), c.get_theta()
            with torch.no_grad():
                p.copy_(torch.from_numpy(before))  # (every step is a first-divergence comparison)
            p.grad = torch.from_numpy(-phi)
            o.step()
            e = _ulps(after, p.detach().numpy(), before)
            assert e <= 4.0, (tick, k, e)
        c.svmpc_forward()
    c.close()


@pytest.mark.parametrize("cls,opt", CASES[::2], ids=IDS[::2])
def test_mpf_steps_follow_torch_and_persist(cls, opt):
    """The filter's optimiser: state and step count persist across optimize() calls (built once in MPF.__init__, mpf.py:24).  One step
    per call, phi read before it (dust_mpf_phi: the same prior and likelihood the step sees), torch's optimiser kept for the whole run."""
    from dust_amd.backend import MpfContext
    from dust_amd.optim import optimizer_config

    rng = np.random.default_rng(3)
    Mp = 32
    x0 = np.stack([1.0 + 0.2 * rng.standard_normal(Mp), 1.0 + 0.2 * rng.standard_normal(Mp)], 1).astype(np.float32)
    bw = 0.1
    m = MpfContext(x0, np.array([3.0, 0.0], np.float32), model="pendulum", uncertain_params=("length", "mass"), obs_std=0.1, init_bw=bw,
                   lr=float(opt["lr"]), optim=optimizer_config(cls, opt))
    m.condition(np.array([0.5], np.float32), np.array([2.9, -0.4], np.float32))
    p = torch.tensor(m.get_particles(), requires_grad=True)
    o = cls([p], **opt)
    for k in range(4):
        before = m.get_particles()
        phi = m.phi(bw)
        m.optimize(None, None, bw, 1)
        after = m.get_particles()
        with torch.no_grad():
            p.copy_(torch.from_numpy(before))
        p.grad = torch.from_numpy(-phi)
        o.step()
        assert _ulps(after, p.detach().numpy(), before) <= 4.0, k
    c2 = m.clone()  # dust_mpf_clone copies the state and the step count
    m.optimize(None, None, bw, 2)
    c2.optimize(None, None, bw, 2)
    assert np.array_equal(m.get_particles(), c2.get_particles())
    m.close()
    c2.close()


@pytest.mark.parametrize("model", ["pendulum", "particle"])
def test_plain_sgd_and_adam_bit_identical(model):
    """SGD(momentum=0, dampening=0, weight_decay=0) and Adam(weight_decay=0, amsgrad=False) given through dust_set_optimizer give the bits of
    dust_config's DUST_OPT_SGD / DUST_OPT_ADAM contexts (the Adam scalars are fp32-exact here: dust_config carries them as floats)."""
    from dust_amd.optim import optimizer_config

    N, S, H = 64, 64, 12
    da = 1 if model == "pendulum" else 2
    lr = 2.0 if model == "pendulum" else 100.0
    pairs = [(dict(optimizer="SGD", lr=lr), optimizer_config(torch.optim.SGD, dict(lr=lr, momentum=0.0, dampening=0.0, weight_decay=0.0))),
             (dict(optimizer="Adam", lr=0.5, adam=(0.875, 0.9990234375, 1e-8)),
              optimizer_config(torch.optim.Adam, dict(lr=0.5, betas=(0.875, 0.9990234375), eps=1e-8, weight_decay=0.0, amsgrad=False)))]
    for legacy, oc in pairs:
        a, rng = _make(model, N, S, H, **legacy)
        b, _ = _make(model, N, S, H, **legacy)
        b.set_optimizer(oc)
        b.set_theta(a.get_theta())
        st = _state(model)
        for t in range(3):
            eps = rng.standard_normal((3, S, N, H, da)).astype(np.float32)
            ra, rb = a.svmpc_tick(st, 3, eps), b.svmpc_tick(st, 3, eps)
            assert np.array_equal(ra[0], rb[0]) and np.array_equal(a.get_theta(), b.get_theta()), (legacy["optimizer"], t)
        a.close()
        b.close()


@pytest.mark.parametrize("cls,opt", CASES, ids=IDS)
def test_tick2_equals_launch_per_iteration(cls, opt):
    """A cfg2-shaped context (N = 1024, H = 30, 5 iterations): the owner-computes one-launch tick (tick2.hpp, state in registers)
    against DUST_NO_TICK2=1, at test_gpu_tick2.py's tolerance; the other context takes over theta and the mixture after every tick.
    The one-launch kernel provably served ticks 2-3 (tick 1 runs plain kernels on both: the prior means do not alias the particles yet)."""
    N, S, H, iters = 1024, 128, 30, 5
    a, rng = _make("pendulum", N, S, H, cls, opt)
    b, _ = _make("pendulum", N, S, H, cls, opt, env={"DUST_NO_TICK2": "1"})
    st = _state("pendulum")
    for t in range(3):
        eps = rng.standard_normal((iters, S, N, H, 1)).astype(np.float32)
        ra, rb = a.svmpc_tick(st, iters, eps=eps), b.svmpc_tick(st, iters, eps=eps)
        assert elemerr(a.get_theta(), b.get_theta()) < 5e-4, t
        assert elemerr(a.get_phi(), b.get_phi()) < 5e-4, t
        b.set_theta(a.get_theta())  # (the prior means alias the particles: they follow; the optimiser state restarts at a roll anyway)
        b.set_a_mat(a.get_a_mat())
        del ra, rb
    from helpers import tick2_ticks_expected

    shape = dict(eps=np.zeros((3, iters)), N=N, H=H, da=1, sigma_p=2.0)  # (what tick2_ticks_expected reads of a scenario)
    assert a.tick_stats()["tick2"] == tick2_ticks_expected(shape, "pend_cfg2") and b.tick_stats()["tick2"] == 0
    a.close()
    b.close()


@pytest.mark.parametrize("cls,opt", [CASES[5], CASES[4], CASES[0]], ids=[IDS[5], IDS[4], IDS[0]])
def test_clone_continues_identically(cls, opt):
    """dust_clone (copy.deepcopy) taken mid-chain - between optimize and forward, with the state slots live - continues bit for bit."""
    import copy

    N, S, H = 64, 64, 15
    a, rng = _make("pendulum", N, S, H, cls, opt)
    st = _state("pendulum")
    a.svmpc_tick(st, 3)
    a.svmpc_tick(st, 3)
    a.svmpc_optimize(st, 2)
    b = copy.deepcopy(a)
    assert b.get_optimizer() == a.get_optimizer()
    for ctx in (a, b):
        ctx.svmpc_optimize(st, 2)
        ctx.svmpc_forward()
        ctx.svmpc_tick(st, 3)
    assert np.array_equal(a.get_theta(), b.get_theta())
    a.close()
    b.close()


def test_set_theta_restarts_state():
    """dust_set_theta is a new parameter tensor: momentum SGD's first step after it is a plain step again (buffer = clone(grad))."""
    from dust_amd.optim import optimizer_config

    N, S, H = 32, 64, 8
    c, rng = _make("pendulum", N, S, H, torch.optim.SGD, dict(lr=0.5, momentum=0.9), env={"DUST_NO_TICK2": "1"})
    st = _state("pendulum")
    c.svmpc_optimize(st, 2)
    th = c.get_theta()
    c.set_theta(th)
    eps = rng.standard_normal((1, S, N, H, 1)).astype(np.float32)
    c.svmpc_optimize(st, 1, eps)
    assert _ulps(c.get_theta(), th + 0.5 * c.get_phi(), th) <= 2.0
    assert c.get_optimizer() == optimizer_config(torch.optim.SGD, dict(lr=0.5, momentum=0.9))
    c.close()


# ---- golden chains: the reference's own SVMPC / MPF run with these optimisers (tests/golden/make_golden_optim.py)
SVMPC_GOLDENS = ["pend_k1_sgdmom_nesterov", "pend_k1_rmsprop_centered_mom", "part_k1_adagrad", "pend_k1_adamw_amsgrad", "pend_k2_rmsprop"]


def _golden_optim(g):
    import json

    from dust_amd.optim import optimizer_config

    return optimizer_config(getattr(torch.optim, str(g["opt_class"])), json.loads(str(g["opt_args"])))


def _golden_ctx(g):
    from dust_amd import Context
    from oracle import grid_4x4_map
    from test_gpu_parity import ctx_kwargs

    kw = ctx_kwargs(g)
    return Context(grid=grid_4x4_map() if kw["model"] == "particle" else None, optim=_golden_optim(g), **kw)


@pytest.mark.parametrize("name", SVMPC_GOLDENS)
def test_steps_vs_reference(golden, name):
    """test_adam_steps_vs_reference for the other optimisers: every step of the reference's own chain from its particles / noise, and
    the restart of the optimiser state at each forward() (SVMPC.roll swaps a new parameter tensor into the group; torch keys the state
    by tensor).  theta after the steps and after the roll is held to 1e-4 element-wise, through pieces and through svmpc_tick, and the
    owner-computes one-launch kernel served the eligible ticks."""
    from helpers import tick2_ticks_expected

    g = golden(name)
    T, K = g["eps"].shape[:2]
    ctxs = []
    for tick_entry in (False, True):
        c = _golden_ctx(g)
        c.set_theta(g["theta0"])
        c.set_prior(g["mu0"], g["mix0"])
        c.set_a_mat(g["a_mat0"])
        for t in range(T):
            params = g["params"][t] if "params" in g else None
            if tick_entry:
                c.svmpc_tick(g["state"][t, 0], K, g["eps"][t], params)
            else:
                c.svmpc_optimize(g["state"][t, 0], K, g["eps"][t], params)
                assert elemerr(c.get_theta(), g["theta_after"][t, K - 1]) < 1e-4, (name, t)
                c.svmpc_forward()
            assert elemerr(c.get_theta(), g["tick_theta_rolled"][t]) < 1e-4, (name, tick_entry, t)
        ctxs.append(c)
    for c in ctxs:
        st = c.tick_stats()
        assert st["tick2"] == tick2_ticks_expected(g, name) and st["replayed"] == 0, (name, st)
        c.close()


@pytest.mark.parametrize("name", ["mpf_pend_rmsprop", "mpf_part_log_adagrad"])
def test_mpf_vs_reference(golden, name):
    """MPF with RMSprop / Adagrad: two filter updates of the reference's own run; the state and step count persist from the first
    optimize() to the second (mpf.py:24); a bare phi() leaves them and a clone carries them.  Held to 1e-4 element-wise, the bound of the
    SVMPC chains: the normalised steps carry phi's rounding differences (summation order, exp / log ulps) into the particles over 2 x n
    steps, while the update arithmetic itself is pinned to a few ulps by test_mpf_steps_follow_torch_and_persist."""
    from dust_amd import MpfContext
    from oracle import grid_4x4_map

    g = golden(name)
    kind = str(g["model_kind"])
    up = ("length", "mass") if kind == "pendulum" else ("mass",)
    bw, ls, n = float(g["bw"]), bool(int(g["log_space"])), int(g["n_steps"])
    m = MpfContext(g["x0"], g["obs0"], model=kind, uncertain_params=up, log_space=ls, obs_std=float(g["obs_std"]), lr=float(g["lr"]),
                   init_bw=bw, grid=grid_4x4_map() if kind == "particle" else None, mass=2.0 if kind == "particle" else 1.0,
                   optim=_golden_optim(g))
    m.optimize(g["action"], g["obs1"], bw, n)
    assert elemerr(m.get_particles(), g["x_final"]) < 1e-4
    m.phi(bw)
    mc = m.clone()
    for mm in (m, mc):
        mm.optimize(g["action2"], g["obs2"], bw, n)
        assert elemerr(mm.get_particles(), g["x_final2"]) < 1e-4
    m.close()
    mc.close()


# ---- the other device paths agree with the plain calls
def _pend_plant(st, a):
    thd = np.float32(np.clip(st[1] + 0.05 * (14.7 * np.sin(st[0]) + 3.0 * np.clip(a, -2, 2)), -8, 8))
    return np.array([st[0] + thd * 0.05, thd], np.float32)


@pytest.mark.parametrize("cls,opt", [CASES[5], CASES[7], CASES[4]], ids=[IDS[5], IDS[7], IDS[4]])
def test_served_loop_is_bit_identical(cls, opt):
    """Closed-loop serving (dust_svmpc_serve_start: the next tick launched ahead, waiting for its plant state) with the optimiser state
    in the one-launch kernel's registers: the same results as the same calls without serving, bit for bit."""
    runs = []
    for serve in (False, True):
        c, _ = _make("pendulum", 256, 128, 30, cls, opt)  # (one context on the device at a time)
        st = _state("pendulum")
        c.svmpc_tick(st, 1)
        if serve:
            c.serve_start(3, 20000.0)
        out = []
        for t in range(20):
            a_seq, pw = c.svmpc_tick(st, 3)
            out.append((a_seq.copy(), pw.copy()))
            st = _pend_plant(st, float(a_seq[0, 0]))
        stats = c.tick_stats()
        if serve:
            c.serve_stop()
        runs.append((out, c.get_theta(), stats))
        c.close()
    (oa, tha, sa), (ob, thb, sb) = runs
    for t, ((a0, p0), (a1, p1)) in enumerate(zip(oa, ob)):
        assert np.array_equal(a0, a1) and np.array_equal(p0, p1), t
    assert np.array_equal(tha, thb)
    assert sa["served"] == 0 and sb["served"] == 20 and sb["replayed"] == 0, sb


@pytest.mark.parametrize("world", [2, 4])
def test_sharded_equals_unsharded(golden, world):
    """Particle sharding on one GPU (DeviceShard + LocalComm: the all-gathers as slice copies) with RMSprop (all three state slots live on
    every shard): every shard ends each tick with the particles of the unsharded context."""
    from dust_amd import Context
    from dust_amd.parallel import DeviceShard, LocalComm, tick
    from test_gpu_parity import ctx_kwargs

    g = golden("pend_k1_rmsprop_centered_mom")
    kw = dict(ctx_kwargs(g), optim=_golden_optim(g))
    T, K = g["eps"].shape[:2]
    ref = Context(**kw)
    ref.set_theta(g["theta0"]); ref.set_prior(g["mu0"]); ref.set_a_mat(g["a_mat0"])
    shards = tuple(DeviceShard(kw, r, world) for r in range(world))
    for s in shards:
        assert s.ctx.get_optimizer() == kw["optim"]
        s.set_state(g["theta0"], g["mu0"], g["a_mat0"])
    for t in range(T):
        ref.svmpc_optimize(g["state"][t, 0], K, g["eps"][t])
        ref.svmpc_forward()
        tick(shards, LocalComm(), g["state"][t, 0], K, g["eps"][t], None, want_outputs=True)
        for s in shards:
            s.sync()
        rt = ref.get_theta()
        for s in shards:
            assert elemerr(s.ctx.get_theta(), rt) < 1e-5, (world, t, s.rank)
    ref.close()


def test_fused_dual_tick_with_rmsprop_filter_equals_its_pieces(monkeypatch):
    """DualSVMPC(fused=True) - dust_dual_tick - with an RMSprop filter (state persisting across the periods) and a momentum-SGD controller,
    against the same pieces called one by one with the same Philox keys: bit-identical over five control periods."""
    from dust_amd import Context, MpfContext
    from dust_amd.optim import optimizer_config

    monkeypatch.setenv("DUST_NO_TICK2", "1")
    N, S, M, H, K, Mp = 64, 32, 4, 12, 2, 48
    rng = np.random.default_rng(9)
    mu = rng.standard_normal((N, H, 1)).astype(np.float32)
    th = (mu + rng.standard_normal((N, H, 1))).astype(np.float32)
    x0 = rng.uniform(0.6, 1.3, (Mp, 2)).astype(np.float32)
    f_opt = optimizer_config(torch.optim.RMSprop, dict(lr=1e-3, momentum=0.3, centered=True))
    c_opt = optimizer_config(torch.optim.SGD, dict(lr=0.5, momentum=0.5))

    def make():
        c = Context(model="pendulum", N=N, S=S, M=M, H=H, kernel="K1", lr=0.5, sigma_a=2.0, sigma_p=2.0, uncertain_params=("length", "mass"),
                    seed=5, optim=c_opt)
        c.set_theta(th); c.set_prior(mu); c.set_a_mat(th)
        m = MpfContext(x0, np.array([3.0, 0.0], np.float32), model="pendulum", uncertain_params=("length", "mass"), obs_std=0.1, lr=1e-3,
                       init_bw=0.1, optim=f_opt)
        return c, m

    ca, ma = make()
    cb, mb = make()
    sa = sb = np.array([3.0, 0.0], np.float32)
    prev = None
    for t in range(5):
        a1, p1, bw1 = ca.dual_tick(ma, sa, prev, K, mpf_steps=6, mpf_bw=None, seed=100 + t)
        if prev is not None:
            bw2 = mb.silverman()
            mb.optimize(prev, sb, bw2, 6)
            assert bw1 == bw2
        params = mb.prior_sample(K * M, 100 + t).reshape(K, M, 2)
        a2, p2 = cb.svmpc_tick(sb, K, None, params)
        assert np.array_equal(a1, a2) and np.array_equal(p1, p2), t
        assert np.array_equal(ma.get_particles(), mb.get_particles()), t
        prev = a1[0].copy()
        sa = sb = _pend_plant(sa, float(a1[0, 0]))
    assert np.array_equal(ca.get_theta(), cb.get_theta())
    for o in (ca, cb, ma, mb):
        o.close()
