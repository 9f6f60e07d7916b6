"""The DuSt-MPC loop over a batch of plants on the device: dust_svmpc_dual_batch_tick (SvmpcBatch.dual_tick, svmpc_prior_batch_kernel)
and dust_amd.controllers.BatchDualSVMPC.

1. - 5. bit for bit (np.array_equal, no tolerance): the fused period against its pieces (dust_mpf_batch_optimize on a clone of the
   filters, dust_svmpc_batch_tick on a clone of the controllers fed params_out), the rows against dust_mpf_prior_sample and the exact
   integer Philox of tests/philox_ref.py, invariance under the slot, the neighbours, the mask and a clone, the launch count, refusals.
   One check in this group is a bound and not np.array_equal: test_component_index_is_the_hosts takes the component index from the
   host's integer Philox (exact) and then holds each row to 6 bw of that component's mean and to 1e-6 of a float64 Box-Muller - the
   device's fp32 log / sin / cos cannot be restated bit for bit in numpy, the construction of test_gpu_amppi_dual.py.  The bit equality
   of the same rows is test_rows_are_the_priors_samples.
6. against the lone path (DualSVMPC(fused=True)): the filters bit for bit, the controllers to rounding - the lone and the batched SVMPC
   kernels add in different orders -, first-divergence form at the tolerances of test_gpu_svmpc_batch.py."""
import copy
import ctypes as C
import importlib.util
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import philox_ref as px
from helpers import elemerr
from test_gpu_svmpc_batch import TOL

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MPF_STEPS = 4
GETTERS = ("THETA", "PRIOR_MEANS", "PRIOR_MIX", "A_MAT", "COSTS", "SCORE", "PHI", "LOG_L", "LOG_P", "A_MIX", "ACTIONS")
CENTRE = dict(length=1.0, mass=1.0, g=9.8, x_icr=0.2, wheel_radius=0.0625, axial_distance=0.475, mass_pole=1.0, mass_cart=1.0, f_mag=1.0)
STATE0 = dict(pendulum=[3.0, 0.0], particle=[-3.0, -3.0, 0.0, 0.0], skid_steer=[0.3, -0.2, 0.4, 0.1, -0.05], cartpole=[0.1, 0.2, 0.15, -0.1])


@pytest.fixture(autouse=True)
def _single_workgroup_filters(monkeypatch):
    """lone filters run the single-workgroup kernel whose arithmetic the batch repeats (the switch is read in dust_mpf_create)"""
    monkeypatch.setenv("DUST_MPF_GRID", "0")


def _L():
    from dust_amd import _lib

    return _lib


def _records(sb):
    L = _L()
    return {n: sb.get(getattr(L, "SVB_" + n)) for n in GETTERS}


def _plant(state, action):
    """a small host plant: any deterministic map does"""
    new = state.copy()
    new[: action.size] += np.float32(0.02) * np.tanh(action)
    new[-1] += np.float32(0.01)
    return new.astype(np.float32)


def _controller_kw(family, up, log, N, S, M, H, opt, kernel, seed=77):
    kw = dict(kernel=kernel, optimizer=opt, seed=seed)
    if family == "pendulum":
        kw.update(model=family, N=N, S=S, M=M, H=H, lr=2.0, sigma_a=2.0, sigma_p=2.0, uncertain_params=up, params_log_space=log)
        return kw, 1.0
    if family == "particle":
        from oracle import grid_4x4_map

        kw.update(model=family, N=N, S=S, M=M, H=H, lr=100.0, sigma_a=5.0, sigma_p=5.0, grid=grid_4x4_map(), uncertain_params=up, params_log_space=log)
        return kw, 1.0
    if family == "skid_steer":
        import skid_cases as sc

        return sc.controller_kwargs(sc.R("dual_batch", N, S, H, M, up, "uniform", None, 0, log=log), lr=0.05, **kw), 0.3
    import cartpole_cases as cc

    return cc.controller_kwargs(cc.R("dual_batch", N, S, H, M, up, "uniform", None, 0, log=log), lr=0.05, **kw), 0.5


def _filter_kw(family, up, log, opt):
    from oracle import grid_4x4_map

    kw = dict(model=family, uncertain_params=up, obs_std=0.2, lr=1e-3 if opt == "Adam" else 1e-6, init_bw=0.05, optimizer=opt, log_space=log)
    if family == "particle":
        kw.update(grid=grid_4x4_map(), mass=2.0)
    if family == "skid_steer":
        kw.update(dt=0.1)
    if family == "cartpole":
        kw.update(dt=0.05)
    return kw


def _setup(family, up, log, N, S, M, H, Mp, opt, kernel, B, seeds, env_ids=None):
    """-> (controller batch, filter batch, states [B, ds], filter keywords).  Environment `e` of `env_ids` (default 0 .. B - 1) gets its
    own particles, prior means, a_mat, filter particles and state, whichever slot it sits in."""
    from dust_amd import Context, MpfContext

    env_ids = list(range(B)) if env_ids is None else env_ids
    kw, scale = _controller_kw(family, up, log, N, S, M, H, opt, kernel)
    da = 1 if family in ("pendulum", "cartpole") else 2
    P = len(up)
    centre = np.array([2.0 if (family == "particle" and k == "mass") else CENTRE[k] for k in up], np.float32)
    th, mu, am, xs, states = [], [], [], [], []
    for e in env_ids:
        rng = np.random.default_rng(1000 + e)
        mu.append((scale * rng.standard_normal((N, H, da))).astype(np.float32))
        th.append((mu[-1] + 2 * scale * rng.standard_normal((N, H, da))).astype(np.float32))
        am.append((scale * rng.standard_normal((N, H, da))).astype(np.float32))
        x0 = (centre * (1.0 + 0.05 * rng.standard_normal((Mp, P)))).astype(np.float32)
        xs.append(np.log(x0) if log else x0)
        states.append((np.array(STATE0[family], np.float32) + 0.01 * rng.standard_normal(len(STATE0[family]))).astype(np.float32))
    L = _L()
    c = Context(**kw)
    sb = c.svmpc_batch(B, seeds=seeds)
    c.close()
    sb.set(L.SVB_THETA, np.stack(th))
    sb.set(L.SVB_PRIOR_MEANS, np.stack(mu))
    sb.set(L.SVB_A_MAT, np.stack(am))
    fkw = _filter_kw(family, up, log, opt)
    m = MpfContext(xs[0], states[0], **fkw)
    mb = m.batch(B)
    m.close()
    mb.set_particles(np.stack(xs))
    states = np.stack(states)
    mb.set_obs(states)
    return sb, mb, states, fkw


# ------------------------------------------------------------------------------------------------ 1. fused equals its pieces
# id, family, uncertain parameters, log space, N, S, M, H, Mp, n_steps, optimiser, kernel, fixed bandwidth (None: Silverman), device noise
PIECES = [
    ("pendulum-P2-M8", "pendulum", ("length", "mass"), False, 3, 16, 8, 6, 48, 3, "SGD", "K1", None, False),
    ("pendulum-P1-M1", "pendulum", ("length",), False, 4, 8, 1, 5, 1, 1, "Adam", "IMQ", 0.05, True),
    ("pendulum-P3-M3", "pendulum", ("g", "length", "mass"), False, 2, 16, 3, 6, 3, 3, "Adam", "K1", None, True),
    ("pendulum-P2-M64", "pendulum", ("length", "mass"), False, 2, 4, 64, 4, 48, 3, "SGD", "K1", 0.05, False),
    ("particle-P1-M3", "particle", ("mass",), False, 3, 16, 3, 6, 48, 3, "SGD", "IMQ", None, False),
    ("skid-P3-M3", "skid_steer", ("x_icr", "wheel_radius", "axial_distance"), False, 4, 16, 3, 6, 3, 3, "Adam", "K1", 0.01, True),
    ("skid-log-P2-M8", "skid_steer", ("x_icr", "wheel_radius"), True, 3, 8, 8, 5, 48, 3, "SGD", "K1", None, False),
    ("cartpole-P4-M8", "cartpole", ("mass_pole", "length", "mass_cart", "f_mag"), False, 4, 16, 8, 6, 48, 3, "SGD", "K1", None, True),
    ("cartpole-P4-M3-adam", "cartpole", ("mass_pole", "length", "mass_cart", "f_mag"), False, 3, 8, 3, 6, 3, 1, "Adam", "IMQ", 0.02, False),
]


@pytest.mark.parametrize("name,family,up,log,N,S,M,H,Mp,n_steps,opt,kernel,bw,device_noise", PIECES, ids=[p[0] for p in PIECES])
def test_fused_period_equals_its_pieces(name, family, up, log, N, S, M, H, Mp, n_steps, opt, kernel, bw, device_noise):
    """three consecutive periods of B = 3 (the first without a filter update); before each, clones of both batches run the pieces"""
    B = 3
    sb, mb, states, _ = _setup(family, up, log, N, S, M, H, Mp, opt, kernel, B, seeds=[7, 11, 5])
    da, P = sb.da, len(up)
    rng = np.random.default_rng(N + S + M)
    prev = None
    for t in range(3):
        sb2, mb2 = sb.clone(), mb.clone()
        eps = None if device_noise else rng.standard_normal((B, n_steps, S, N, H, da)).astype(np.float32)
        keys = [100 + t + (b << 32) for b in range(B)]
        a1, pw1, rows, bwu = sb.dual_tick(mb, states, prev, n_steps=n_steps, eps=eps, mpf_steps=MPF_STEPS, mpf_bw=bw, seeds=keys,
                                          want_params=True, keep_actions=True)
        assert rows.shape == (B, n_steps, M, P)
        if prev is None:
            assert (bwu == 0.0).all(), t
        else:
            _, bw2 = mb2.optimize(prev, states, bw, MPF_STEPS)
            assert np.array_equal(bwu, bw2), (t, bwu, bw2)
            if bw is not None:
                assert (bwu == np.float32(bw)).all()
        a2, pw2 = sb2.tick(states, n_steps, eps=eps, params=rows, keep_actions=True)
        assert np.array_equal(mb.get_particles(), mb2.get_particles()) and np.array_equal(mb.get_prior_bw(), mb2.get_prior_bw()), t
        assert np.array_equal(a1, a2) and np.array_equal(pw1, pw2), t
        r1, r2 = _records(sb), _records(sb2)
        for k in GETTERS:
            assert np.array_equal(r1[k], r2[k]), (t, k)
        assert np.isfinite(a1).all() and np.isfinite(rows).all() and np.isfinite(r1["THETA"]).all() and np.isfinite(mb.get_particles()).all(), t
        sb2.close()
        mb2.close()
        prev = a1[:, 0].copy()
        states = np.stack([_plant(states[b], prev[b]) for b in range(B)])
    sb.close()
    mb.close()


# ------------------------------------------------------------------------------------------------ 2. the rows are the prior's
@pytest.mark.parametrize("name,family,up,log,N,S,M,H,Mp,n_steps,opt,kernel,bw,device_noise", [PIECES[0], PIECES[2], PIECES[6], PIECES[7]],
                         ids=[PIECES[i][0] for i in (0, 2, 6, 7)])
def test_rows_are_the_priors_samples(name, family, up, log, N, S, M, H, Mp, n_steps, opt, kernel, bw, device_noise):
    """params_out[b] = dust_mpf_prior_sample(f_b, n_steps M, prior_seeds[b]) for a lone filter f_b given environment b's particles and
    prior bandwidths as they are after the period's update"""
    from dust_amd import MpfContext

    B = 3
    sb, mb, states, fkw = _setup(family, up, log, N, S, M, H, Mp, opt, kernel, B, seeds=[7, 11, 5])
    prev = None
    for t in range(2):
        keys = [(1 << 40) + 31 * t + (b << 32) for b in range(B)]
        a, _, rows, _ = sb.dual_tick(mb, states, prev, n_steps=n_steps, mpf_steps=MPF_STEPS, mpf_bw=bw, seeds=keys, want_params=True)
        x, pb = mb.get_particles(), mb.get_prior_bw()
        for b in range(B):
            f = MpfContext(x[b], states[b], **fkw)
            f.set_particles(x[b])
            f.set_prior_bw(pb[b])
            assert np.array_equal(rows[b].reshape(n_steps * M, len(up)), f.prior_sample(n_steps * M, keys[b])), (t, b)
            f.close()
        prev = a[:, 0].copy()
        states = np.stack([_plant(states[b], prev[b]) for b in range(B)])
    sb.close()
    mb.close()


def test_component_index_is_the_hosts():
    """n_steps = 3, M = 8, Mp = 3, P = 2, component means 100 bw apart: the component of row i = it M + m of environment b is
    (philox4x32_10(i, 0x6d7066, 0, 0; prior_seeds[b])[0] Mp) >> 32 in exact integer arithmetic (tests/philox_ref.py), and |z| < 6 for any
    draw (24-bit uniforms: sqrt(-2 ln 2^-25) = 5.89), so every row lies within 6 bw of ITS mean - of ITS environment's particles"""
    from dust_amd import Context, MpfContext

    B, n_steps, M, Mp, P, bw = 2, 3, 8, 3, 2, 0.01
    kw, _ = _controller_kw("pendulum", ("length", "mass"), False, 3, 16, M, 6, "SGD", "K1")
    c = Context(**kw)
    sb = c.svmpc_batch(B, seeds=[1, 2])
    c.close()
    means = np.stack([(1.0 + b + 100.0 * bw * np.arange(Mp)[:, None] * np.ones((1, P))).astype(np.float32) for b in range(B)])
    m = MpfContext(means[0], np.array([3.0, 0.0], np.float32), model="pendulum", uncertain_params=("length", "mass"), init_bw=bw)
    mb = m.batch(B)
    m.close()
    mb.set_particles(means)
    keys = [20260, 20260 + (1 << 32)]
    states = np.tile(np.array([3.0, 0.0], np.float32), (B, 1))
    rows = sb.dual_tick(mb, states, None, n_steps=n_steps, seeds=keys, want_params=True)[2]
    n = n_steps * M
    for b in range(B):
        ctr = np.zeros((n, 4), np.uint64)
        ctr[:, 0], ctr[:, 1] = np.arange(n), 0x6D7066
        k = ((px.philox4x32_10(ctr, keys[b])[:, 0].astype(np.uint64) * np.uint64(Mp)) >> np.uint64(32)).astype(np.int64)
        assert set(k.tolist()) == {0, 1, 2}
        ctr[:, 1], ctr[:, 2] = 0x6D7067, 1
        z = px.normal4(ctr, keys[b])[:, :P]
        got = rows[b].reshape(n, P)
        assert (np.abs(got - means[b][k]) <= 6.0 * bw).all(), b
        # (the draw itself against the host's float64 Box-Muller, the bound of test_gpu_amppi_dual.py test_component_index_is_the_hosts: half
        # an ulp of a value below 8 is 2.4e-7, the device's fp32 log / sin / cos add < 1e-7 at bw = 0.01)
        assert np.abs(got - (means[b][k] + bw * z)).max() < 1e-6, b
    assert not np.array_equal(rows[0] - 1.0, rows[1] - 2.0)  # (other keys: other components)
    sb.close()
    mb.close()


# ------------------------------------------------------------------------------------------------ 3. invariance
SHAPE = dict(family="pendulum", up=("length", "mass"), log=False, N=3, S=16, M=3, H=6, Mp=48, opt="Adam", kernel="K1")
N_STEPS, TICKS = 2, 3


def _state_of(sb, mb):
    out = _records(sb)
    out["x"], out["prior_bw"] = mb.get_particles(), mb.get_prior_bw()
    return out


def _run(env_ids, device_noise, active=None, clone_after=None, ticks=TICKS):
    """`ticks` periods of a batch whose slots hold the environments `env_ids` (each with its own seed, keys, noise, plant trajectory);
    -> per period the records of every slot (and those of a pair of clones taken after period `clone_after`)"""
    B = len(env_ids)
    sb, mb, states, _ = _setup(B=B, seeds=[900 + e for e in env_ids], env_ids=env_ids, **SHAPE)
    N, S, H = SHAPE["N"], SHAPE["S"], SHAPE["H"]
    out, out_twin, twin = [], [], None
    prev = None
    for t in range(ticks):
        eps = None if device_noise else np.stack([np.random.default_rng(50 * e + t).standard_normal((N_STEPS, S, N, H, 1)).astype(np.float32)
                                                  for e in env_ids])
        keys = [5000 + t + (e << 32) for e in env_ids]
        args = dict(n_steps=N_STEPS, eps=eps, mpf_steps=MPF_STEPS, seeds=keys, active=active, want_params=True, keep_actions=True)
        a, pw, rows, bwu = sb.dual_tick(mb, states, prev, **args)
        out.append(dict(_state_of(sb, mb), a_seq=a, pw=pw, rows=rows, bw=bwu))
        if twin is not None:
            a2, pw2, rows2, bw2 = twin[0].dual_tick(twin[1], states, prev, **args)
            out_twin.append(dict(_state_of(*twin), a_seq=a2, pw=pw2, rows=rows2, bw=bw2))
        if clone_after == t:
            twin = (sb.clone(), mb.clone())
        # (open loop: the states and previous actions of an environment do not depend on what its batch computed)
        prev = np.stack([np.array([0.3 * np.sin(e + t)], np.float32) for e in env_ids])
        states = np.stack([_plant(states[i], prev[i]) for i in range(B)])
    for o in (sb, mb) + (twin or ()):
        o.close()
    return out, out_twin


@pytest.mark.parametrize("device_noise", [False, True], ids=["recorded", "device"])
def test_an_environment_does_not_depend_on_its_batch(device_noise):
    me, others = 9, [20, 21, 22, 23]
    alone, _ = _run([me], device_noise)

    def same(rec, slot):
        for t in range(TICKS):
            for k, v in alone[t].items():
                assert np.array_equal(rec[t][k][slot], v[0]), (slot, t, k)

    for slot in (0, 2, 4):
        rec, twin = _run(others[:slot] + [me] + others[slot:], device_noise, clone_after=0)
        same(rec, slot)
        for t in (1, 2):  # the clones taken mid-loop continue as their sources do, every slot
            for k, v in rec[t].items():
                assert np.array_equal(twin[t - 1][k], v), (t, k)
    # beside inactive neighbours, which keep everything and whose output rows are not written
    mask = np.array([0, 0, 1, 0, 0], np.uint8)
    ids = others[:2] + [me] + others[2:]
    rec, _ = _run(ids, device_noise, active=mask)
    same(rec, 2)
    sb, mb, _, _ = _setup(B=5, seeds=[900 + e for e in ids], env_ids=ids, **SHAPE)
    keep_x, keep_bw = mb.get_particles(), mb.get_prior_bw()
    L = _L()
    keep = {n: sb.get(getattr(L, "SVB_" + n)) for n in ("THETA", "PRIOR_MEANS", "PRIOR_MIX", "A_MAT")}
    sb.close()
    mb.close()
    off = [0, 1, 3, 4]
    for t in range(TICKS):
        for k in ("a_seq", "pw", "rows", "bw"):
            assert np.isnan(rec[t][k][off]).all(), (t, k)
        assert np.array_equal(rec[t]["x"][off], keep_x[off]) and np.array_equal(rec[t]["prior_bw"][off], keep_bw[off]), t
        for k, v in keep.items():
            assert np.array_equal(rec[t][k][off], v[off]), (t, k)


@pytest.mark.parametrize("device_noise", [False, True], ids=["recorded", "device"])
def test_a_sleeper_wakes_up_where_it_was(device_noise):
    """optimiser state, optimiser step count and stream position of an inactive environment (and its filter's) are untouched: switched on
    after two periods of its neighbours, it computes its own first periods - against the same environment alone"""
    ids = [20, 9, 21]
    B = len(ids)
    alone, _ = _run([9], device_noise, ticks=2)
    sb, mb, states, _ = _setup(B=B, seeds=[900 + e for e in ids], env_ids=ids, **SHAPE)
    N, S, H = SHAPE["N"], SHAPE["S"], SHAPE["H"]
    sentinel = np.float32(-77.0)
    lib, FP = _L().load(), _L().FP
    st0 = states.copy()
    for t in range(2):  # the neighbours' periods: the sleeper's output rows keep the sentinel
        a = np.full((B, H, 1), sentinel, np.float32)
        pw = np.full((B, N), sentinel, np.float32)
        rows = np.full((B, N_STEPS, SHAPE["M"], 2), sentinel, np.float32)
        bwu = np.full(B, sentinel, np.float32)
        keys = np.array([7000 + t + (e << 32) for e in ids], np.uint64)
        mask = np.array([1, 0, 1], np.uint8)
        prev = None if t == 0 else np.full((B, 1), 0.1, np.float32)
        st = lib.dust_svmpc_dual_batch_tick(sb._h, mb._h, states.ctypes.data_as(FP), None if prev is None else prev.ctypes.data_as(FP), N_STEPS, None, 0,
                                            MPF_STEPS, -1.0, keys.ctypes.data_as(C.POINTER(C.c_uint64)), mask.ctypes.data_as(C.POINTER(C.c_ubyte)),
                                            a.ctypes.data_as(FP), pw.ctypes.data_as(FP), rows.ctypes.data_as(FP), bwu.ctypes.data_as(FP))
        assert st == 0
        assert (a[1] == sentinel).all() and (pw[1] == sentinel).all() and (rows[1] == sentinel).all() and bwu[1] == sentinel
        assert not (a[[0, 2]] == sentinel).any() and not (rows[[0, 2]] == sentinel).any() and not (bwu[[0, 2]] == sentinel).any()
        states = states + np.float32(0.01)
    states = st0
    prev = None
    for t in range(2):  # the sleeper's own first two periods, with the inputs of _run([9])
        eps = None if device_noise else np.stack([np.random.default_rng(50 * e + t).standard_normal((N_STEPS, S, N, H, 1)).astype(np.float32) for e in ids])
        keys = [5000 + t + (e << 32) for e in ids]
        a, pw, rows, bwu = sb.dual_tick(mb, states, prev, n_steps=N_STEPS, eps=eps, mpf_steps=MPF_STEPS, seeds=keys, active=np.array([0, 1, 0], np.uint8),
                                        want_params=True, keep_actions=True)
        got = dict(_state_of(sb, mb), a_seq=a, pw=pw, rows=rows, bw=bwu)
        for k, v in alone[t].items():
            assert np.array_equal(got[k][1], v[0]), (t, k)
        prev = np.stack([np.array([0.3 * np.sin(e + t)], np.float32) for e in ids])
        states = np.stack([_plant(states[i], prev[i]) for i in range(B)])
    sb.close()
    mb.close()


# ------------------------------------------------------------------------------------------------ 4. launch count
def _counts(nb):
    """profile and stats counters added by one period with a filter update at nb environments, Silverman bandwidths, nothing read back"""
    sb, mb, states, _ = _setup(B=nb, seeds=list(range(nb)), **SHAPE)
    keys = [1 + (b << 32) for b in range(nb)]
    a = sb.dual_tick(mb, states, None, n_steps=N_STEPS, seeds=keys)[0]
    sb.ctx.profile(True)
    s0 = mb.stats()
    out = sb.dual_tick(mb, states + np.float32(0.01), a[:, 0].copy(), n_steps=N_STEPS, seeds=[k + 1 for k in keys], mpf_steps=MPF_STEPS, want_outputs=False)
    assert all(o is None for o in out)  # (nothing read back: the call returned without waiting for the device)
    prof, s1 = sb.ctx.profile_get(), mb.stats()
    sb.ctx.profile(False)
    assert np.isfinite(sb.get(_L().SVB_THETA)).all() and np.isfinite(mb.get_particles()).all()
    sb.close()
    mb.close()
    return {k: v[1] for k, v in prof.items()}, {k: s1[k] - s0[k] for k in s0}


def test_launch_count_does_not_depend_on_B():
    p1, s1 = _counts(1)
    p5, s5 = _counts(5)
    assert p1 == p5 and s1 == s5, (p1, p5, s1, s5)
    assert p1 == dict(svmpc_batch_kernel=1), p1  # (the tick is counted under DUST_K_SVMPC_BATCH, and nothing else on the controller's side)
    assert s1 == dict(launches=2, calls=1), s1  # (Silverman's rule and the update)


# ------------------------------------------------------------------------------------------------ 5. refusals
def test_refusals_leave_both_batches_as_they_were():
    from dust_amd import Context, MpfContext

    L = _L()
    B = 2
    sb, mb, states, fkw = _setup(B=B, seeds=[1, 2], **SHAPE)
    keys = [1, 2]
    a = sb.dual_tick(mb, states, None, n_steps=1, seeds=keys, keep_actions=True)[0]  # (records exist: every getter answers)
    prev = a[:, 0].copy()
    before = _state_of(sb, mb)
    sb.ctx.profile(True)
    s0 = mb.stats()

    def fresh(batch, filt):
        """what a pair that has not ticked yet answers: the controllers' settable tensors, the filters' particles, bandwidths and counters"""
        out = {n: batch.get(getattr(L, "SVB_" + n)) for n in ("THETA", "PRIOR_MEANS", "PRIOR_MIX", "A_MAT")}
        out["x"], out["prior_bw"], out["stats"] = filt.get_particles(), filt.get_prior_bw(), filt.stats()
        return out

    def refused(status, batch, filt, *args, match=None, **kw):
        mine = fresh(batch, filt)
        with pytest.raises(L.DustError) as e:
            batch.dual_tick(filt, *args, **kw)
        assert e.value.status == status, (e.value.status, str(e.value))
        assert match is None or match in str(e.value), str(e.value)
        now = _state_of(sb, mb)
        for k, v in before.items():
            assert np.array_equal(now[k], v), k
        assert sb.ctx.profile_get() == {} and mb.stats() == s0
        now = fresh(batch, filt)  # (the pair of the call itself, where it is another one)
        for k, v in mine.items():
            assert now[k] == v if k == "stats" else np.array_equal(now[k], v), k
        if batch is not sb:  # ... which still has no record of a tick
            with pytest.raises(L.DustError):
                batch.get(L.SVB_COSTS)

    ok = dict(n_steps=1, seeds=keys)
    refused(L.ERR_UNSUPPORTED, sb, mb, states, prev, flags=L.STORE_STATES, **ok)
    refused(L.ERR_UNSUPPORTED, sb, mb, states, prev, flags=L.STORE_F16, **ok)
    refused(L.ERR_UNSUPPORTED, sb, mb, states, prev, flags=L.EPS_F16, **ok)
    refused(L.ERR_INVALID, sb, mb, states, prev, n_steps=0, seeds=keys)
    refused(L.ERR_INVALID, sb, mb, states, prev, mpf_steps=-1, **ok)
    refused(L.ERR_INVALID, sb, mb, states, prev, n_steps=1, seeds=None)
    refused(L.ERR_INVALID, sb, mb, None, prev, **ok)
    refused(L.ERR_INVALID, sb, mb, states, prev, mpf_steps=4097, **ok)  # (mpfb_update_check)
    mb3b = MpfContext(np.ones((16, 2), np.float32), states[0], **fkw).batch(3)
    refused(L.ERR_INVALID, sb, mb3b, np.tile(states[0], (3, 1))[:2], prev, **ok)  # n_env differs
    m1 = MpfContext(np.ones((16, 1), np.float32), states[0], model="pendulum", uncertain_params=("length",))
    mb1 = m1.batch(B)
    refused(L.ERR_INVALID, sb, mb1, states, prev, **ok)  # parameter columns differ (dual_pair_check)
    # a controller that samples nothing (dim_p = 0), and one with sigma-point weights: no batched form
    kw, _ = _controller_kw("pendulum", None, False, SHAPE["N"], SHAPE["S"], 1, SHAPE["H"], "SGD", "K1")
    c0 = Context(**kw)
    sb0 = c0.svmpc_batch(B)
    refused(L.ERR_INVALID, sb0, mb, states, prev, **ok)
    kw, _ = _controller_kw("pendulum", ("length", "mass"), False, SHAPE["N"], SHAPE["S"], 5, SHAPE["H"], "SGD", "K1")
    cs = Context(**kw)
    sbs = cs.svmpc_batch(B)
    sbs.ctx.set_param_weights(np.full(5, 0.2, np.float32))
    sbs.ctx.set_sigma_scale(3.0)
    refused(L.ERR_UNSUPPORTED, sbs, mb, states, prev, **ok)
    # a cart-pole controller over a pendulum filter of as many columns
    kw, _ = _controller_kw("cartpole", ("mass_pole", "length"), False, 3, 8, 3, 6, "SGD", "K1")
    cc_ = Context(**kw)
    sbc = cc_.svmpc_batch(B)
    refused(L.ERR_INVALID, sbc, mb, np.zeros((B, 4), np.float32), None, match="a cart-pole controller takes a cart-pole filter", **ok)
    # as many columns of the same family on both sides, but other names or another order (dual_pair_check's two loops)
    closers = []

    def filters(family, up):
        x = np.tile(np.array([CENTRE[k] for k in up], np.float32), (16, 1))
        f = MpfContext(x, np.array(STATE0[family], np.float32), **_filter_kw(family, up, False, "SGD"))
        fb = f.batch(B)
        closers.extend([fb, f])
        return fb

    kw, _ = _controller_kw("skid_steer", ("x_icr", "wheel_radius"), False, 3, 8, 3, 5, "SGD", "K1")
    ck = Context(**kw)
    sbk = ck.svmpc_batch(B)
    st5, pv2 = np.tile(np.array(STATE0["skid_steer"], np.float32), (B, 1)), np.full((B, 2), 0.1, np.float32)
    for up in (("wheel_radius", "x_icr"), ("x_icr", "axial_distance")):
        for pv in (None, pv2):
            refused(L.ERR_INVALID, sbk, filters("skid_steer", up), st5, pv, match="uncertain skid-steer parameters", **ok)
    st4, pv1 = np.tile(np.array(STATE0["cartpole"], np.float32), (B, 1)), np.full((B, 1), 0.1, np.float32)
    for up in (("length", "mass_pole"), ("mass_pole", "mass_cart")):
        for pv in (None, pv1):
            refused(L.ERR_INVALID, sbc, filters("cartpole", up), st4, pv, match="uncertain cart-pole parameters", **ok)
    for o in closers + [sbk, ck]:
        o.close()
    # ... and the same call goes through afterwards
    sb.ctx.profile(False)
    a2 = sb.dual_tick(mb, states, prev, mpf_steps=MPF_STEPS, **ok)[0]
    assert np.isfinite(a2).all() and mb.stats()["calls"] == s0["calls"] + 1
    for o in (sbc, cc_, sbs, cs, sb0, c0, mb1, m1, mb3b, sb, mb):
        o.close()


def test_an_amppi_batch_and_an_svmpc_batch_share_one_filter_batch():
    """two controller batches on their own streams tick on ONE filter batch in turn, nothing read back in between: the filters' particles
    equal those of a filter batch updated alone with the same inputs (every tick waits for the one before it through the filters' event)"""
    from dust_amd import Context

    B = 2
    sb, mb, states, _ = _setup(B=B, seeds=[1, 2], **SHAPE)
    ref = mb.clone()
    ca = Context(model="pendulum", N=1, S=64, M=1, H=8, temperature=100.0, alpha=0.01, sigma_a=2.0, uncertain_params=("length", "mass"), seed=3)
    ab = ca.amppi_batch(B)
    keys = [1, 2]
    prev = np.full((B, 1), 0.2, np.float32)
    for t in range(4):
        st = states + np.float32(0.01 * t)
        if t % 2 == 0:
            sb.dual_tick(mb, st, prev, n_steps=1, seeds=keys, mpf_steps=MPF_STEPS, mpf_bw=0.05, want_outputs=False)
        else:
            ab.dual_tick(mb, st, prev, seeds=keys, mpf_steps=MPF_STEPS, mpf_bw=0.05, roll=1, want_outputs=False)
        ref.optimize(prev, st, 0.05, MPF_STEPS)
    assert np.array_equal(mb.get_particles(), ref.get_particles()) and np.array_equal(mb.get_prior_bw(), ref.get_prior_bw())
    assert np.isfinite(sb.get(_L().SVB_THETA)).all() and np.isfinite(ab.get_a_seq()).all()
    for o in (ab, ca, sb, mb, ref):
        o.close()


# ------------------------------------------------------------------------------------------------ 6. against the lone path
def _example():
    path = os.path.join(ROOT, "examples", "svmpc_dual_batch_example.py")
    spec = importlib.util.spec_from_file_location("svmpc_dual_batch_example", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _mirror(family, opt, B, seed):
    """-> (BatchDualSVMPC of B environments, [DualSVMPC(fused=True, seed=seed + (b << 32))] over the same configuration, states [B, ds])"""
    from dust_amd.controllers import BatchDualSVMPC, DualSVMPC, MultiDISCO
    from dust_amd.costs import PendulumQuadCos, QuadraticCost
    from dust_amd.inference import MPF, SVMPC, BatchSVMPC, ExponentiatedUtility, GaussianLikelihood, get_gmm
    from dust_amd.kernels import RBFKernel
    from dust_amd.models import CartPoleModel, PendulumModel

    N, S, M, H, Mp = 4, 16, 3, 6, 48
    g = torch.Generator().manual_seed(3)
    if family == "pendulum":
        up, sig, temp, alpha, centre, lr = ("length", "mass"), 2.0, 1.0, 1.0, torch.tensor([1.0, 1.0]), 0.5
        state = torch.tensor([3.0, 0.0])
    else:
        import cartpole_cases as cc

        # (columns of one scale: Silverman's rule pools them, and a drawn pole mass must stay positive)
        up, sig, temp, alpha, centre, lr = ("mass_cart", "mass_pole", "length"), cc.SIGMA_A, 4.0, 0.25, torch.tensor([1.0, 1.0, 1.0]), 0.05
        state = torch.tensor(cc.STATE0)
    mu = 0.4 * torch.randn(N, H, 1, generator=g)
    th = mu + 0.3 * sig * torch.randn(N, H, 1, generator=g)
    x0 = centre * (1.0 + 0.05 * torch.randn(B, Mp, len(up), generator=g))
    states = state[None] + 0.01 * torch.randn(B, state.numel(), generator=g)
    cov = sig ** 2 * torch.eye(1)
    opt_kw = dict(optimizer_class=torch.optim.Adam, lr=0.1) if opt == "Adam" else dict(optimizer_class=torch.optim.SGD, lr=lr)

    def parts(b):
        if family == "pendulum":
            model, cost = PendulumModel(uncertain_params=up), PendulumQuadCos()
        else:
            import cartpole_cases as cc

            model, cost = CartPoleModel(uncertain_params=up), QuadraticCost(cc.GOAL, cc.W_STATE, cc.W_TERM, cc.W_CTRL)
        ctrl = MultiDISCO(model.observation_space, model.action_space, H, N, S, temperature=temp, a_cov=cov, inst_cost_fn=cost.inst_cost,
                          term_cost_fn=cost.term_cost, params_sampling=True, params_samples=M, seed=40 + b)
        ctrl.a_mat = th.clone()
        ctrl.return_rollouts = False
        mpf = MPF(init_particles=x0[b].clone(), likelihood=GaussianLikelihood(initial_obs=states[b], obs_std=0.2, model=model, log_space=False),
                  optimizer_class=torch.optim.SGD, lr=1e-6, bw=0.05)
        kw = dict(init_particles=th.clone(), prior=get_gmm(mu, torch.ones(N), cov), kernel=RBFKernel(), n_particles=N, n_steps=2,
                  likelihood=ExponentiatedUtility(alpha=alpha, n_samples=S, controller=ctrl, model=model), **opt_kw)
        return kw, mpf

    lones = []
    for b in range(B):
        kw, mpf = parts(b)
        lones.append(DualSVMPC(SVMPC(**kw), mpf, mpf_steps=MPF_STEPS, fused=True, seed=seed + (b << 32)))
    kw, mpf = parts(0)
    loop = BatchDualSVMPC(BatchSVMPC(B, seeds=[40 + b for b in range(B)], **kw), mpf, mpf_steps=MPF_STEPS, seed=seed, init_particles=x0)
    return loop, lones, states


@pytest.mark.parametrize("family,opt", [("pendulum", "SGD"), ("pendulum", "Adam"), ("cartpole", "SGD"), ("cartpole", "Adam")])
def test_class_against_lone_objects(family, opt):
    """BatchDualSVMPC (B = 3) and three DualSVMPC(fused=True, seed=seed + (b << 32)) under one prescribed, open-loop sequence of states and
    previous actions over three periods, device-drawn noise under equal keys (environment b's stream is its lone controller's).  Filters (48 particles: the single-workgroup kernel): particles and last_bw bit for bit, every period.  Controllers:
    first-divergence form - after every period the lone objects take the batch's particles over - at the tolerances of
    test_gpu_svmpc_batch.py test_batch_svmpc_agrees_with_B_svmpc_objects (a_seq and theta 25 TOL element-wise, p_weights 2e-3 absolute).
    A deep copy of the class taken after the first period continues bit-equal."""
    B, seed = 3, 20260
    loop, lones, states = _mirror(family, opt, B, seed)
    twin = None
    rng = np.random.default_rng(4)
    for t in range(3):
        if t > 0:
            actions = torch.from_numpy((0.3 * rng.standard_normal((B, 1))).astype(np.float32))
            states = states + torch.from_numpy((0.02 * rng.standard_normal(tuple(states.shape))).astype(np.float32))
            for o in [loop] + ([twin] if twin is not None else []):
                o.step(actions, states)
            for b, lo in enumerate(lones):
                lo.step(actions[b], states[b])
        a_b, pw_b = loop.forward(states)
        if twin is not None:
            a_t, pw_t = twin.forward(states)
            assert torch.equal(a_t, a_b) and torch.equal(pw_t, pw_b) and torch.equal(twin.theta, loop.theta), t
            assert torch.equal(twin.dyn_particles, loop.dyn_particles), t
        outs = [lo.forward(states[b]) for b, lo in enumerate(lones)]
        x = loop.dyn_particles
        for b, lo in enumerate(lones):
            assert torch.equal(x[b], lo.dyn_particles), (t, b)
            if t > 0:
                assert float(loop.last_bw[b]) == np.float32(lo.last_bw), (t, b)
            ea, ep = elemerr(a_b[b].numpy(), outs[b][0].numpy()), float((pw_b[b] - outs[b][1]).abs().max())
            et = elemerr(loop.theta[b].numpy(), lo.theta.numpy())
            print("%s %s t %d b %d: a_seq %.1e  p_weights %.1e  theta %.1e" % (family, opt, t, b, ea, ep, et))
            assert ea < 25 * TOL and ep < 2e-3 and et < 25 * TOL, (t, b, ea, ep, et)
        for b, lo in enumerate(lones):  # first-divergence form: the lone objects take the batch's particles over
            lo.svmpc.theta = loop.theta[b]
        if t == 0:
            twin = copy.deepcopy(loop)
            assert twin._mb is not loop._mb and twin.svmpc._batch is not loop.svmpc._batch
    assert loop.ticks == 3 and loop._t == 3 and loop.prior_keys(3)[1] == seed + (1 << 32) + 3


def test_a_refused_call_keeps_the_keys_and_the_noted_update():
    L = _L()
    loop, _, states = _mirror("pendulum", "SGD", 2, 5)
    a, _ = loop.forward(states)
    loop.step(a[:, 0], states + 0.01)
    t, pend = loop._t, loop._pending
    loop.mpf_steps = -1  # (dust_svmpc_dual_batch_tick refuses a negative step count)
    with pytest.raises(L.DustError):
        loop.forward(states + 0.01)
    assert loop._t == t and loop._pending is pend and pend is not None
    loop.mpf_steps = MPF_STEPS
    a, _ = loop.forward(states + 0.01)
    assert torch.isfinite(a).all() and loop._t == t + 1 and loop._pending is None and loop.last_bw is not None


def test_the_example_runs():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "svmpc_dual_batch_example.py"), "--envs", "3", "--ticks", "3", "--samples", "16",
                          "--particles", "3", "--horizon", "8", "--mpf-particles", "16"], capture_output=True, text=True, timeout=300,
                         env=dict(os.environ, PYTHONPATH=ROOT))
    assert out.returncode == 0, out.stderr[-2000:]
    assert "3 ticks of 3 pendulums" in out.stdout
