"""Per-environment filter hyper-parameters on the device: dust_mpf_batch_set_hyper / _get_hyper (MpfBatch.set_hyper / .hyper), the rows
forms of the batched filter kernels (mpf_optimize_rows_kernel, mpf_silverman_rows_kernel) and every entry they reach through the one
launch site of a batched update - dust_mpf_batch_optimize, the dual ticks and the dual episodes of both controller batches - up to
BatchDualSVMPC.set_filter_hyper and the drivers.  Cases: tests/mpf_sweep_cases.py.

Every comparison is np.array_equal, with one exception: test_row_against_the_reference holds the middle environment of three, whose ROW
is a fixture's configuration, to the reference's own filter (tests/golden/mpf_pend.npz, mpf_pend_adam.npz, mpf_part_log.npz) at the
bounds tests/test_gpu_parity.py test_mpf / test_mpf_adam hold a lone filter to."""
import copy
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import mpf_sweep_cases as sw
from helpers import elemerr, relerr

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = 1e-5  # (tests/test_gpu_parity.py)


@pytest.fixture(autouse=True)
def _single_workgroup_filters(monkeypatch):
    """lone filters run the single-workgroup kernel whose arithmetic the batch repeats (the switch is read in dust_mpf_create)"""
    monkeypatch.setenv("DUST_MPF_GRID", "0")


def _L():
    from dust_amd import _lib

    return _lib


def _kw(case, row=None):
    from oracle import grid_4x4_map

    kw = sw.filter_kw(case, row)
    if kw["model"] == "particle":
        kw["grid"] = grid_4x4_map()
    return kw


def _batch(case, Mp, envs, rows=None, proto_row=None):
    """a filter batch whose slot s holds environment envs[s] (its own particles and observation); the prototype is created with
    `proto_row`'s values (default: the case's), `rows` are set on the batch -> (batch, observations [B, ds])"""
    from dust_amd import MpfContext

    xs, obs = zip(*[sw.particles(case, Mp, e) for e in envs])
    m = MpfContext(xs[0], obs[0], **_kw(case, proto_row))
    mb = m.batch(len(envs))
    m.close()
    mb.set_particles(np.stack(xs))
    mb.set_obs(np.stack(obs))
    if rows is not None:
        mb.set_hyper(rows)
    return mb, np.stack(obs)


def _update(mb, case, envs, t, obs, bw=None, active=None):
    """update t of every slot's environment -> (grad_norms, bw_used, the new observations)"""
    acts, new = zip(*[sw.update_inputs(case, e, t, obs[s]) for s, e in enumerate(envs)])
    gn, bwu = mb.optimize(np.stack(acts), np.stack(new), bw, sw.MPF_STEPS, active=active)
    return gn, bwu, np.stack(new)


def _call_bw(row):
    return row["bw"] if row["bw"] > 0 else None


def _hyper_list(h):
    return [{k: float(r[k]) for k in sw.FIELDS} for r in h]


# ------------------------------------------------------------------------------------------------ 1. an environment against a one-environment batch
@pytest.mark.parametrize("case,Mp", sw.GRID, ids=sw.GRID_IDS)
def test_environment_equals_a_filter_created_with_its_row(case, Mp):
    """environment b of five under the table's rows against a ONE-environment batch (no rows) of a prototype filter created with row b's
    obs_std, lr and bw_scale and called with bw = rows[b].bw when that is > 0, else Silverman's rule: particles, prior bandwidths,
    bw_used and grad_norms over four consecutive updates - the fourth shows the optimiser slots and the step count the third left"""
    rows = sw.rows(case)
    envs = list(range(sw.B))
    mb, obs = _batch(case, Mp, envs, rows)
    ones = [_batch(case, Mp, [b], None, proto_row=rows[b]) for b in envs]
    obs1 = [o for _, o in ones]
    s0 = mb.stats()
    for t in range(4):
        gn, bwu, obs = _update(mb, case, envs, t, obs)
        x, pb = mb.get_particles(), mb.get_prior_bw()
        assert np.isfinite(x).all() and np.isfinite(gn).all() and (bwu > 0).all()
        for b in envs:
            one = ones[b][0]
            gn1, bw1, obs1[b] = _update(one, case, [b], t, obs1[b], bw=_call_bw(rows[b]))
            assert np.array_equal(obs1[b][0], obs[b])
            assert np.array_equal(x[b], one.get_particles()[0]), (t, b)
            assert np.array_equal(pb[b], one.get_prior_bw()[0]), (t, b)
            assert bwu[b] == bw1[0] and np.array_equal(gn[b], gn1[0]), (t, b, bwu[b], bw1[0])
            assert (pb[b] == bwu[b]).all(), (t, b)  # (the refreshed prior bandwidths report the bandwidth of the update)
        assert bwu[4] == np.float32(rows[4]["bw"])
        if Mp > 1:
            assert bwu[3] != bwu[0] and bwu[4] != bwu[0]
    s1 = mb.stats()
    assert {k: s1[k] - s0[k] for k in s0} == dict(launches=8, calls=4)  # (the rows' Silverman launch and the update, per call)
    for o in [mb] + [o for o, _ in ones]:
        o.close()


# ------------------------------------------------------------------------------------------------ 2. rows equal to the prototype's
@pytest.mark.parametrize("fixed", [None, 0.05], ids=["silverman", "fixed"])
@pytest.mark.parametrize("case,Mp", [("pend_sgd", 65), ("pend_adam_log", 3), ("part_mass_log", 130), ("pend_p1_sgd", 1)])
def test_rows_equal_to_the_prototypes_are_the_batch_without_rows(case, Mp, fixed):
    """all rows at the prototype's values: on Silverman's rule against bw <= 0, at a fixed c against bw = c"""
    envs = [0, 1, 2]
    row = dict(sw.proto_row(case), bw=0.0 if fixed is None else sw.f32(fixed))
    mb, obs = _batch(case, Mp, envs, [row] * 3)
    ref, obs_r = _batch(case, Mp, envs)
    for t in range(3):
        gn, bwu, obs = _update(mb, case, envs, t, obs)
        gn_r, bwu_r, obs_r = _update(ref, case, envs, t, obs_r, bw=None if fixed is None else row["bw"])
        assert np.array_equal(gn, gn_r) and np.array_equal(bwu, bwu_r), t
        assert np.array_equal(mb.get_particles(), ref.get_particles()) and np.array_equal(mb.get_prior_bw(), ref.get_prior_bw()), t
    mb.close()
    ref.close()


# ------------------------------------------------------------------------------------------------ 3. one field, one environment
@pytest.mark.parametrize("field", sw.FIELDS)
@pytest.mark.parametrize("case,Mp", [("pend_sgd", 65), ("pend_adam_log", 3), ("part_mass_log", 65)])
def test_one_field_of_one_row_moves_that_environment_alone(case, Mp, field):
    """a rows path that ignored a field would pass every comparison of two rows paths: here one field of environment 1's row differs
    from the prototype's, and its particles - nobody else's - leave those of the batch whose rows are all the prototype's"""
    envs = [0, 1, 2]
    p = sw.proto_row(case)
    rows = [dict(p), dict(p, **{field: sw.other_value(case, field)}), dict(p)]
    mb, obs = _batch(case, Mp, envs, rows)
    ref, obs_r = _batch(case, Mp, envs, [dict(p)] * 3)
    for t in range(2):
        _, bwu, obs = _update(mb, case, envs, t, obs)
        _, bwu_r, obs_r = _update(ref, case, envs, t, obs_r)
    x, xr = mb.get_particles(), ref.get_particles()
    assert not np.array_equal(x[1], xr[1]), field
    assert np.array_equal(x[0], xr[0]) and np.array_equal(x[2], xr[2]), field
    assert bwu[0] == bwu_r[0] and bwu[2] == bwu_r[2] and (field not in ("bw", "bw_scale") or bwu[1] != bwu_r[1])
    mb.close()
    ref.close()


# ------------------------------------------------------------------------------------------------ 4. slots, masks and clones
@pytest.mark.parametrize("case,Mp", [("pend_adam_log", 65), ("part_mass_log", 3)])
def test_an_environment_does_not_depend_on_its_slot_its_neighbours_or_a_clone(case, Mp):
    """environment 7 under row 1 (lr x 4), alone in slots 0 / 2 / 4 of five beside INACTIVE neighbours that hold other rows and other
    particles, and from a clone taken after the first update: the same bits as in a one-environment batch under that row"""
    rows = sw.rows(case)
    mine = rows[1]
    one, obs1 = _batch(case, Mp, [7], [mine])
    want = []
    for t in range(3):
        gn, bwu, obs1 = _update(one, case, [7], t, obs1)
        want.append((gn[0], bwu[0], one.get_particles()[0], one.get_prior_bw()[0]))
    one.close()
    for slot in (0, 2, 4):
        envs = [20, 21, 22, 23, 24]
        envs[slot] = 7
        rr = [rows[(s + 2) % 5] for s in range(5)]
        rr[slot] = mine
        mb, obs = _batch(case, Mp, envs, rr)
        active = [1 if s == slot else 0 for s in range(5)]
        x0 = mb.get_particles()
        for t in range(3):
            if t == 1:
                twin = mb.clone()
                assert _hyper_list(twin.hyper) == _hyper_list(mb.hyper)
                mb.close()
                mb = twin
            gn, bwu, new = _update(mb, case, envs, t, obs, active=active)
            obs[slot] = new[slot]
            x = mb.get_particles()
            assert np.array_equal(gn[slot], want[t][0]) and bwu[slot] == want[t][1], (slot, t)
            assert np.array_equal(x[slot], want[t][2]) and np.array_equal(mb.get_prior_bw()[slot], want[t][3]), (slot, t)
            for s in range(5):
                if s != slot:
                    assert np.array_equal(x[s], x0[s]) and np.isnan(bwu[s]), (slot, t, s)
        mb.close()


# ------------------------------------------------------------------------------------------------ 5. set and get
def test_set_get_clear_and_what_stays():
    case, Mp = "pend_adam_log", 65
    envs = list(range(sw.B))
    rows = sw.rows(case)
    mb, obs = _batch(case, Mp, envs)
    ref, obs_r = _batch(case, Mp, envs)
    p = sw.proto_row(case)
    assert _hyper_list(mb.hyper) == [p] * sw.B  # (no rows: the prototype's values, bw 0)
    assert mb.hyper["lr"].dtype == np.float64
    _, _, obs = _update(mb, case, envs, 0, obs)
    _, _, obs_r = _update(ref, case, envs, 0, obs_r)
    x, pb, st = mb.get_particles(), mb.get_prior_bw(), mb.stats()
    mb.set_hyper(rows)
    assert _hyper_list(mb.hyper) == rows
    assert np.array_equal(mb.get_particles(), x) and np.array_equal(mb.get_prior_bw(), pb) and mb.stats() == st  # (nothing else is touched)
    mb.set_hyper(np.array([(r["lr"], r["obs_std"]) for r in rows], dtype=[("lr", np.float64), ("obs_std", np.float32)]))
    assert _hyper_list(mb.hyper) == [dict(p, lr=r["lr"], obs_std=r["obs_std"]) for r in rows]  # (fields left out: the prototype's)
    with pytest.raises(ValueError):
        mb.set_hyper(rows[:2])
    with pytest.raises(ValueError):
        mb.set_hyper([dict(r, sigma=1.0) for r in rows])
    mb.set_hyper(rows)
    twin, deep = mb.clone(), copy.deepcopy(mb)
    assert _hyper_list(twin.hyper) == rows and _hyper_list(deep.hyper) == rows
    mb.set_hyper(None)
    assert _hyper_list(mb.hyper) == [p] * sw.B and _hyper_list(twin.hyper) == rows
    # back to the no-rows bits: optimiser slots, step counts and bandwidths went through the set / clear untouched
    for t in (1, 2):
        gn, bwu, obs = _update(mb, case, envs, t, obs)
        gn_r, bwu_r, obs_r = _update(ref, case, envs, t, obs_r)
        assert np.array_equal(gn, gn_r) and np.array_equal(bwu, bwu_r), t
        assert np.array_equal(mb.get_particles(), ref.get_particles()), t
    # ... while the clones kept the rows
    g1, b1, _ = _update(twin, case, envs, 1, _batch_obs(case, Mp, envs, 0))
    g2, b2, _ = _update(deep, case, envs, 1, _batch_obs(case, Mp, envs, 0))
    assert np.array_equal(g1, g2) and np.array_equal(b1, b2) and b1[4] == np.float32(rows[4]["bw"])
    assert np.array_equal(twin.get_particles(), deep.get_particles())
    for o in (mb, ref, twin, deep):
        o.close()


def _batch_obs(case, Mp, envs, upto):
    """the observations after update `upto` of every environment (what _update returned then)"""
    obs = np.stack([sw.particles(case, Mp, e)[1] for e in envs])
    for t in range(upto + 1):
        obs = np.stack([sw.update_inputs(case, e, t, obs[s])[1] for s, e in enumerate(envs)])
    return obs


# ------------------------------------------------------------------------------------------------ 6. against the reference
@pytest.mark.parametrize("name", ["mpf_pend", "mpf_pend_adam", "mpf_part_log"])
def test_row_against_the_reference(golden, name):
    """the configuration of a fixture of the reference's own filter as the ROW of the middle environment of three; the prototype holds
    other values for all four fields and the neighbours hold other rows.  Bounds: those of tests/test_gpu_parity.py test_mpf /
    test_mpf_adam (elemerr TOL on the particles, relerr TOL / 2e-4 on the two calls' grad_norms)."""
    from dust_amd import MpfContext
    from oracle import grid_4x4_map

    g = golden(name)
    kind = str(g["model_kind"])
    up = ("length", "mass") if kind == "pendulum" else ("mass",)
    bw, ls, n = float(g["bw"]), bool(int(g["log_space"])), int(g["n_steps"])
    lr, std = sw.f32(g["lr"]), sw.f32(g["obs_std"])
    m = MpfContext(g["x0"], g["obs0"], model=kind, uncertain_params=up, log_space=ls, obs_std=3.0 * std, lr=0.37 * lr, bw_scale=2.5,
                   init_bw=bw, grid=grid_4x4_map() if kind == "particle" else None, mass=2.0 if kind == "particle" else 1.0,
                   optimizer=str(g["optimizer"]))
    mb = m.batch(3)
    m.close()
    mine = dict(lr=lr, obs_std=std, bw=sw.f32(bw), bw_scale=1.0)
    mb.set_hyper([dict(lr=2.0 * lr, obs_std=0.5 * std, bw=0.0, bw_scale=0.7), mine, dict(lr=0.5 * lr, obs_std=2.0 * std, bw=sw.f32(2.0 * bw), bw_scale=1.0)])
    acts, o1, o2 = np.tile(g["action"], (3, 1)), np.tile(g["obs1"], (3, 1)), np.tile(g["obs2"], (3, 1))
    gn, bwu = mb.optimize(acts, o1, None, n)
    x = mb.get_particles()
    assert bwu[1] == np.float32(bw)
    assert elemerr(x[1], g["x_final"]) < TOL and relerr(gn[1], g["grad_norms"]) < TOL
    assert elemerr(x[0], g["x_final"]) > 10 * TOL and elemerr(x[2], g["x_final"]) > 10 * TOL  # (the neighbours are elsewhere)
    gn2, _ = mb.optimize(np.tile(g["action2"], (3, 1)), o2, None, n)
    assert elemerr(mb.get_particles()[1], g["x_final2"]) < TOL and relerr(gn2[1], g["grad_norms2"]) < 2e-4
    mb.close()


# ------------------------------------------------------------------------------------------------ 7. through the dual ticks
SV = dict(family="pendulum", up=("length", "mass"), log=False, N=3, S=16, M=3, H=6, Mp=65, opt="Adam", kernel="K1")
SV_PART = dict(family="particle", up=("mass",), log=False, N=3, S=16, M=3, H=6, Mp=3, opt="SGD", kernel="IMQ")


def _sv_rows(shape, B):
    """the table's row kinds over the filter prototype of tests/test_gpu_svmpc_dual_batch.py (_filter_kw)"""
    lr = sw.f32(1e-3 if shape["opt"] == "Adam" else 1e-6)
    p = dict(lr=lr, obs_std=sw.f32(0.2), bw=0.0, bw_scale=1.0)
    kinds = [dict(p), dict(p, lr=sw.f32(4.0 * lr)), dict(p, obs_std=sw.f32(0.1)), dict(p, bw_scale=0.5), dict(p, bw=sw.f32(0.05))]
    return [kinds[(b + 1) % 5] for b in range(B)]


@pytest.mark.parametrize("shape", [SV, SV_PART], ids=["pendulum", "particle"])
def test_svmpc_dual_tick_with_rows_equals_its_pieces_and_its_one_environment_pairs(shape):
    """dust_svmpc_dual_batch_tick with rows on the filter batch, three periods of B = 4: the fused period against
    dust_mpf_batch_optimize with the same rows, then dust_svmpc_batch_tick fed params_out, on clones; and environment b against the
    one-environment pair whose filter batch holds row b"""
    import test_gpu_svmpc_dual_batch as sd

    B, n_steps = 4, 2
    seeds = [7, 11, 5, 3]
    rows = _sv_rows(shape, B)
    sb, mb, states, _ = sd._setup(B=B, seeds=seeds, **shape)
    mb.set_hyper(rows)
    ones = []
    for b in range(B):
        s1, m1, st1, _ = sd._setup(B=1, seeds=[seeds[b]], env_ids=[b], **shape)
        m1.set_hyper([rows[b]])
        assert np.array_equal(st1[0], states[b])
        ones.append((s1, m1))
    prev = None
    for t in range(3):
        sb2, mb2 = sb.clone(), mb.clone()
        keys = [100 + t + (b << 32) for b in range(B)]
        s0 = mb.stats()
        a1, pw1, par, bwu = sb.dual_tick(mb, states, prev, n_steps=n_steps, mpf_steps=sw.MPF_STEPS, seeds=keys, want_params=True, keep_actions=True)
        s1 = mb.stats()
        assert {k: s1[k] - s0[k] for k in s0} == dict(launches=0 if prev is None else 2, calls=1), t
        if prev is None:
            assert (bwu == 0.0).all()
        else:
            _, bw2 = mb2.optimize(prev, states, None, sw.MPF_STEPS)
            assert np.array_equal(bwu, bw2) and (bwu > 0).all(), (t, bwu, bw2)
            fixed = [b for b in range(B) if rows[b]["bw"] > 0]
            assert fixed and all(bwu[b] == np.float32(rows[b]["bw"]) for b in fixed)
        assert np.array_equal(mb.get_particles(), mb2.get_particles()) and np.array_equal(mb.get_prior_bw(), mb2.get_prior_bw()), t
        eps = sb.get(_L().SVB_ACTIONS)  # (the fused tick kept its actions; the pieces' tick draws the same noise from the same position)
        a2, pw2 = sb2.tick(states, n_steps, params=par, keep_actions=True)
        assert np.array_equal(a1, a2) and np.array_equal(pw1, pw2), t
        assert np.array_equal(eps, sb2.get(_L().SVB_ACTIONS)) and np.array_equal(sb.get(_L().SVB_THETA), sb2.get(_L().SVB_THETA)), t
        for b, (s_1, m_1) in enumerate(ones):
            a_b, pw_b, par_b, bw_b = s_1.dual_tick(m_1, states[b:b + 1], None if prev is None else prev[b:b + 1], n_steps=n_steps, mpf_steps=sw.MPF_STEPS,
                                                   seeds=[keys[b]], want_params=True)
            assert np.array_equal(a_b[0], a1[b]) and np.array_equal(pw_b[0], pw1[b]) and np.array_equal(par_b[0], par[b]), (t, b)
            assert bw_b[0] == bwu[b] and np.array_equal(m_1.get_particles()[0], mb.get_particles()[b]), (t, b)
        sb2.close()
        mb2.close()
        prev = a1[:, 0].copy()
        states = np.stack([sd._plant(states[b], prev[b]) for b in range(B)])
    for o in [sb, mb] + [o for pair in ones for o in pair]:
        o.close()


def _amppi_rows(family, B):
    import amppi_dual_cases as ac

    f = ac.FILTER[family]
    p = dict(lr=sw.f32(f["lr"]), obs_std=sw.f32(f["obs_std"]), bw=0.0, bw_scale=1.0)
    kinds = [dict(p), dict(p, lr=sw.f32(4.0 * p["lr"])), dict(p, obs_std=sw.f32(0.5 * p["obs_std"])), dict(p, bw_scale=0.5), dict(p, bw=sw.f32(0.05))]
    return [kinds[(b + 2) % 5] for b in range(B)]


@pytest.mark.parametrize("family,mode,S,H,Mp", [("pendulum", "extended", 65, 8, 65), ("particle", "single", 64, 10, 3)])
def test_amppi_dual_tick_with_rows_equals_its_pieces_and_its_one_environment_pairs(family, mode, S, H, Mp):
    """dust_amppi_dual_batch_tick with rows on the filter batch (B = 3, three periods): the filters against dust_mpf_batch_optimize with the
    same rows on a clone, the tick against dust_amppi_batch_update fed params_out on a clone; environment b against the one-environment
    pair (its noise seed, its sequence, its particles, row b)"""
    import test_gpu_amppi_dual_batch as ab

    B = ab.B
    rows = _amppi_rows(family, B)
    pairs, batch, mb, states, rng = ab._batch_pair(family, mode, S, H, Mp)
    mb.set_hyper(rows)
    a0, x0 = batch.get_a_seq(), mb.get_particles()
    ones = []
    for b in range(B):
        b1 = pairs[b][0].amppi_batch(1, seeds=[ab.SEEDS[b]])
        b1.set_a_seq(a0[b:b + 1])
        m1 = pairs[b][1].batch(1)
        m1.set_particles(x0[b:b + 1])
        m1.set_obs(states[b:b + 1])
        m1.set_hyper([rows[b]])
        ones.append((b1, m1))
    shared = mode == "single"
    prev = None
    for t in range(3):
        tb, tm = batch.clone(), mb.clone()
        keys = [100 + t + (b << 32) for b in range(B)]
        actions = (batch.get_a_seq()[:, None] + 0.5 * rng.standard_normal((B, S, H, batch.da))).astype(np.float32)
        s0 = mb.stats()
        costs, omega, aseq, par, bwu = batch.dual_tick(mb, states, prev, actions, shared_params=shared, mpf_steps=ab.MPF_STEPS, seeds=keys, roll=1,
                                                       want_params=True)
        s1 = mb.stats()
        # (the rows' Silverman launch and the update; `single` stages one drawn row per environment in a launch of the filter side's)
        assert {k: s1[k] - s0[k] for k in s0} == dict(launches=(0 if prev is None else 2) + (1 if shared else 0), calls=1), t
        if prev is not None:
            _, bw2 = tm.optimize(prev, states, None, ab.MPF_STEPS)
            assert np.array_equal(bwu, bw2) and (bwu > 0).all(), t
        assert np.array_equal(mb.get_particles(), tm.get_particles()) and np.array_equal(mb.get_prior_bw(), tm.get_prior_bw()), t
        c2, o2, a2, _ = tb.update(states, actions, params=par, shared_params=shared)
        assert np.array_equal(costs, c2) and np.array_equal(omega, o2) and np.array_equal(aseq, a2), t
        for b, (b1, m1) in enumerate(ones):
            c_b, o_b, a_b, p_b, bw_b = b1.dual_tick(m1, states[b:b + 1], None if prev is None else prev[b:b + 1], actions[b:b + 1], shared_params=shared,
                                                    mpf_steps=ab.MPF_STEPS, seeds=[keys[b]], roll=1, want_params=True)
            assert np.array_equal(c_b[0], costs[b]) and np.array_equal(o_b[0], omega[b]) and np.array_equal(a_b[0], aseq[b]), (t, b)
            assert np.array_equal(p_b[0], par[b]) and (prev is None or bw_b[0] == bwu[b]), (t, b)
            assert np.array_equal(m1.get_particles()[0], mb.get_particles()[b]), (t, b)
        tb.close()
        tm.close()
        prev = aseq[:, 0].copy()
        states = np.stack([ab._env_plant(b, states[b], prev[b]) for b in range(B)])
    for o in [batch, mb] + [o for pair in ones for o in pair] + [o for p in pairs for o in p[:2]]:
        o.close()


# ------------------------------------------------------------------------------------------------ 8. through the dual episodes
def _plant_rows(shape, B):
    true = dict(length=0.8, mass=1.25 if shape["family"] == "pendulum" else 3.0)
    return np.tile(np.array([true[k] for k in shape["up"]], np.float32), (B, 1)) * (1.0 + 0.02 * np.arange(B, dtype=np.float32)[:, None])


@pytest.mark.parametrize("shape", [SV, SV_PART], ids=["pendulum", "particle"])
def test_svmpc_dual_episode_with_rows_equals_its_periods(shape):
    """dust_svmpc_dual_batch_episode with rows set (B = 4, T = 3) against T dust_svmpc_dual_batch_tick calls on clones fed the recorded
    states and actions: actions, weights, bw_out per environment, both batches afterwards, the filter side's launch count"""
    import test_gpu_svmpc_dual_batch as sd

    B, T, n_steps = 4, 3, 2
    rows = _sv_rows(shape, B)
    sb, mb, states, _ = sd._setup(B=B, seeds=[7, 11, 5, 3], **shape)
    mb.set_hyper(rows)
    sb2, mb2 = sb.clone(), mb.clone()
    keys = np.array([[500 + t + (b << 32) for b in range(B)] for t in range(T)], np.uint64)
    plant = _plant_rows(shape, B)
    s0 = mb.stats()
    xs, acts, pw, bw, a_seq = sb.dual_episode(mb, states, T, n_steps, None, mpf_steps=sw.MPF_STEPS, seeds=keys, plant_params=plant)
    s1 = mb.stats()
    assert {k: s1[k] - s0[k] for k in s0} == dict(launches=2 * (T - 1), calls=T)
    x, a = states, None
    for t in range(T):
        a_t, pw_t, _, bw_t = sb2.dual_tick(mb2, x, a, n_steps=n_steps, mpf_steps=sw.MPF_STEPS, seeds=keys[t])
        assert np.array_equal(a_t[:, 0], acts[t]) and np.array_equal(pw_t, pw[t]), t
        assert np.array_equal(bw_t, bw[t]), (t, bw_t, bw[t])
        x, a = xs[t], acts[t]
    assert np.array_equal(a_t, a_seq)
    fixed = [b for b in range(B) if rows[b]["bw"] > 0]
    assert (bw[0] == 0).all() and (bw[1:] > 0).all() and all((bw[1:, b] == np.float32(rows[b]["bw"])).all() for b in fixed)
    silver = [b for b in range(B) if rows[b]["bw"] <= 0]
    assert len({float(bw[1, b]) for b in silver}) == len(silver)  # (Silverman's rule per environment)
    L = _L()
    assert np.array_equal(mb.get_particles(), mb2.get_particles()) and np.array_equal(mb.get_prior_bw(), mb2.get_prior_bw())
    assert np.array_equal(sb.get(L.SVB_THETA), sb2.get(L.SVB_THETA))
    # one further period on both: the pending pair, the optimiser slots and step counts
    k2 = [900 + (b << 32) for b in range(B)]
    one = sb.dual_tick(mb, xs[-1], acts[-1], n_steps=n_steps, mpf_steps=sw.MPF_STEPS, seeds=k2)
    two = sb2.dual_tick(mb2, xs[-1], acts[-1], n_steps=n_steps, mpf_steps=sw.MPF_STEPS, seeds=k2)
    assert all(np.array_equal(u, v) for u, v in zip(one, two) if u is not None)
    assert np.array_equal(mb.get_particles(), mb2.get_particles())
    for o in (sb, mb, sb2, mb2):
        o.close()


def test_svmpc_dual_simulate_with_rows_equals_its_periods():
    """dust_svmpc_dual_batch_simulate with rows set, one warm-up period (optimize without forward, a zero action) and three control
    periods, against dust_svmpc_dual_batch_optimize / _tick on clones fed the recorded states and actions"""
    import test_gpu_svmpc_dual_batch as sd

    shape, B, T, n_steps = SV, 4, 4, 2
    rows = _sv_rows(shape, B)
    sb, mb, states, _ = sd._setup(B=B, seeds=[7, 11, 5, 3], **shape)
    mb.set_hyper(rows)
    sb2, mb2 = sb.clone(), mb.clone()
    keys = np.array([[700 + t + (b << 32) for b in range(B)] for t in range(T)], np.uint64)
    xs, acts, pw, bw, costs, loss, status, n_run, a_seq = sb.dual_simulate(mb, states, T, n_steps, None, mpf_steps=sw.MPF_STEPS, seeds=keys,
                                                                           plant_params=_plant_rows(shape, B), warm_up=1)
    assert (n_run == T).all() and (status == 0).all() and (acts[0] == 0).all() and np.isfinite(costs).all()
    x, a = states, None
    for t in range(T):
        if t < 1:
            _, bw_t = sb2.dual_optimize(mb2, x, a, n_steps=n_steps, mpf_steps=sw.MPF_STEPS, seeds=keys[t])
        else:
            a_t, pw_t, _, bw_t = sb2.dual_tick(mb2, x, a, n_steps=n_steps, mpf_steps=sw.MPF_STEPS, seeds=keys[t])
            assert np.array_equal(a_t[:, 0], acts[t]) and np.array_equal(pw_t, pw[t]), t
        assert np.array_equal(bw_t, bw[t]), (t, bw_t, bw[t])
        x, a = xs[t], acts[t]
    assert np.array_equal(mb.get_particles(), mb2.get_particles()) and np.array_equal(mb.get_prior_bw(), mb2.get_prior_bw())
    assert np.array_equal(sb.get(_L().SVB_THETA), sb2.get(_L().SVB_THETA))
    for o in (sb, mb, sb2, mb2):
        o.close()


@pytest.mark.parametrize("family,mode,S,H,Mp", [("pendulum", "extended", 65, 8, 65), ("particle", "single", 64, 10, 3)])
def test_amppi_dual_episode_with_rows_equals_its_periods(family, mode, S, H, Mp):
    """dust_amppi_dual_batch_episode with rows set against its periods as dual ticks on clones (tests/test_gpu_amppi_dual_episode.py)"""
    import test_gpu_amppi_dual_episode as ae

    batch, mb, states, plant = ae._setup(family, mode, S, H, Mp, optimizer="Adam")
    rows = _amppi_rows(family, ae.B)
    mb.set_hyper(rows)
    tb, tm = batch.clone(), mb.clone()
    if ae.SCALE[0] is not None:
        tb.ctx.set_sigma_scale(ae.SCALE[0])
    keys = ae._keys(900)
    s0 = mb.stats()
    xs, acts, costs, omega, bwu, a_seq = batch.dual_episode(mb, states, ae.T, None, shared_params=mode == "single", mpf_steps=ae.MPF_STEPS, seeds=keys,
                                                            roll_steps=1, plant_params=plant)
    s1 = mb.stats()
    assert {k: s1[k] - s0[k] for k in s0} == dict(launches=2 * (ae.T - 1) + (ae.T if mode == "single" else 0), calls=ae.T)
    ticks = ae._ticks(tb, tm, states, None, xs, acts, keys, mode, None)
    for t, (c_t, o_t, s_t, b_t) in enumerate(ticks):
        assert np.array_equal(c_t, costs[t]) and np.array_equal(o_t, omega[t]), t
        assert np.array_equal(s_t[:, 0], acts[t]) and np.array_equal(b_t, bwu[t]), (t, b_t, bwu[t])
    fixed = [b for b in range(ae.B) if rows[b]["bw"] > 0]
    assert fixed and all((bwu[1:, b] == np.float32(rows[b]["bw"])).all() for b in fixed)
    ae._same_state(ae._state_of(batch, mb), ae._state_of(tb, tm))
    for o in (batch, mb, tb, tm):
        o.close()


# ------------------------------------------------------------------------------------------------ 9. launch counts
def _filter_launches(B, rows_of):
    """filter-side launches and calls of one dust_mpf_batch_optimize and one dual tick with an update at B environments"""
    import test_gpu_svmpc_dual_batch as sd

    sb, mb, states, _ = sd._setup(B=B, seeds=list(range(B)), **SV)
    mb.set_hyper(rows_of(B))
    sb.ctx.profile(True)
    s0 = mb.stats()
    mb.optimize(np.full((B, 1), 0.1, np.float32), states, None, sw.MPF_STEPS)
    s1 = mb.stats()
    out = sb.dual_tick(mb, states + np.float32(0.01), np.full((B, 1), 0.2, np.float32), n_steps=1, seeds=list(range(1, B + 1)), mpf_steps=sw.MPF_STEPS,
                       want_outputs=False)
    assert all(o is None for o in out)
    s2, prof = mb.stats(), sb.ctx.profile_get()
    assert np.isfinite(mb.get_particles()).all()
    sb.close()
    mb.close()
    return ({k: s1[k] - s0[k] for k in s0}, {k: s2[k] - s1[k] for k in s0}, {k: v[1] for k, v in prof.items()})


def test_launch_count_depends_neither_on_B_nor_on_the_rows():
    p = dict(lr=sw.f32(2e-3), obs_std=sw.f32(0.15), bw=0.0, bw_scale=0.8)
    kinds = {"table": lambda B: _sv_rows(SV, B), "all fixed": lambda B: [dict(p, bw=sw.f32(0.05))] * B, "all silverman": lambda B: [dict(p, bw=0.0)] * B}
    for name, rows_of in kinds.items():
        for B in (1, 5):
            opt, tick, prof = _filter_launches(B, rows_of)
            assert opt == dict(launches=2, calls=1) and tick == dict(launches=2, calls=1), (name, B, opt, tick)
            assert prof == dict(svmpc_batch_kernel=1), (name, B, prof)  # (one controller launch per period)


# ------------------------------------------------------------------------------------------------ 10. refusals
def test_refusals_come_ahead_of_any_staging_or_launch():
    import test_gpu_svmpc_dual_batch as sd
    from dust_amd import Context, MpfContext

    L = _L()
    B = 3
    rows = _sv_rows(SV, B)
    sb, mb, states, _ = sd._setup(B=B, seeds=[1, 2, 3], **SV)
    mb.set_hyper(rows)
    keys = [1, 2, 3]
    a = sb.dual_tick(mb, states, None, n_steps=1, seeds=keys, keep_actions=True)[0]
    prev = a[:, 0].copy()
    ca = Context(model="pendulum", N=1, S=64, M=1, H=8, temperature=100.0, alpha=0.01, sigma_a=2.0, uncertain_params=("length", "mass"), seed=3)
    ab = ca.amppi_batch(B)
    ab.dual_tick(mb, states, None, seeds=keys, roll=0)
    sb.ctx.profile(True)
    ab.ctx.profile(True)

    def snap():
        return dict(sd._state_of(sb, mb), a_seq=ab.get_a_seq(), hyper=mb.hyper, stats=mb.stats())

    before = snap()

    def refused(status, call, match=None):
        with pytest.raises(L.DustError) as e:
            call()
        assert e.value.status == status, (e.value.status, str(e.value))
        assert match is None or match in str(e.value), str(e.value)
        now = snap()
        for k, v in before.items():
            assert now[k] == v if k == "stats" else np.array_equal(now[k], v), k
        assert sb.ctx.profile_get() == {} and ab.ctx.profile_get() == {}

    # a positive call bandwidth while rows are set: every entry
    T = 2
    tk = np.arange(1, T * B + 1, dtype=np.uint64).reshape(T, B)
    plant = np.tile(np.array([0.8, 1.25], np.float32), (B, 1))
    msg = "the rows carry the bandwidths"
    refused(L.ERR_INVALID, lambda: mb.optimize(prev, states, 0.05, sw.MPF_STEPS), msg)
    refused(L.ERR_INVALID, lambda: sb.dual_tick(mb, states, prev, n_steps=1, seeds=keys, mpf_bw=0.05), msg)
    refused(L.ERR_INVALID, lambda: sb.dual_tick(mb, states, None, n_steps=1, seeds=keys, mpf_bw=0.05), msg)
    refused(L.ERR_INVALID, lambda: sb.dual_optimize(mb, states, prev, n_steps=1, seeds=keys, mpf_bw=0.05), msg)
    refused(L.ERR_INVALID, lambda: sb.dual_episode(mb, states, T, 1, prev, mpf_steps=2, mpf_bw=0.05, seeds=tk, plant_params=plant), msg)
    refused(L.ERR_INVALID, lambda: sb.dual_simulate(mb, states, T, 1, prev, mpf_steps=2, mpf_bw=0.05, seeds=tk, plant_params=plant), msg)
    refused(L.ERR_INVALID, lambda: ab.dual_tick(mb, states, prev, seeds=keys, mpf_bw=0.05), msg)
    refused(L.ERR_INVALID, lambda: ab.dual_episode(mb, states, T, prev, mpf_steps=2, mpf_bw=0.05, seeds=tk, plant_params=plant), msg)
    # invalid rows, one per invalid field: the stored rows stay
    for field, value in sw.INVALID:
        bad = [dict(r) for r in rows]
        bad[1][field] = value
        refused(L.ERR_INVALID, lambda: mb.set_hyper(bad), "row 1")
    # what still stands: controller rows are refused by the dual entries, filter rows or not
    hy = sb.get_hyper()
    sb.set_hyper(hy)
    refused(L.ERR_UNSUPPORTED, lambda: sb.dual_tick(mb, states, prev, n_steps=1, seeds=keys), "no per-environment hyper-parameters")
    refused(L.ERR_UNSUPPORTED, lambda: sb.dual_episode(mb, states, T, 1, prev, mpf_steps=2, seeds=tk, plant_params=plant))
    sb.set_hyper(None)
    # ... and the same calls go through afterwards
    sb.ctx.profile(False)
    ab.ctx.profile(False)
    assert np.isfinite(sb.dual_tick(mb, states, prev, n_steps=1, seeds=keys, mpf_steps=2)[0]).all()
    assert np.isfinite(ab.dual_tick(mb, states, prev, seeds=keys, mpf_steps=2)[2]).all()
    for o in (ab, ca, sb, mb):
        o.close()
    # skid-steer and cart-pole filter batches take no rows
    for family, up in (("skid_steer", ("x_icr", "wheel_radius")), ("cartpole", ("mass_pole", "length"))):
        x = np.tile(np.array([sd.CENTRE[k] for k in up], np.float32), (16, 1))
        f = MpfContext(x, np.array(sd.STATE0[family], np.float32), **sd._filter_kw(family, up, False, "SGD"))
        fb = f.batch(2)
        h0, x0, st0 = fb.hyper, fb.get_particles(), fb.stats()
        with pytest.raises(L.DustError) as e:
            fb.set_hyper([dict(lr=1e-3), dict(lr=2e-3)])
        assert e.value.status == L.ERR_UNSUPPORTED and "skid-steer or cart-pole" in str(e.value), str(e.value)
        assert np.array_equal(fb.hyper, h0) and np.array_equal(fb.get_particles(), x0) and fb.stats() == st0
        fb.set_hyper(None)  # (clearing is always allowed)
        fb.close()
        f.close()


# ------------------------------------------------------------------------------------------------ 11. classes and drivers
def _loop(B, seed, envs, x0, states, mpf_bw=None):
    """BatchDualSVMPC over the Pendulum parts of tests/test_gpu_svmpc_dual_batch.py _mirror, environment envs[s] in slot s"""
    from dust_amd.controllers import BatchDualSVMPC, MultiDISCO
    from dust_amd.costs import PendulumQuadCos
    from dust_amd.inference import MPF, BatchSVMPC, ExponentiatedUtility, GaussianLikelihood, get_gmm
    from dust_amd.kernels import RBFKernel
    from dust_amd.models import PendulumModel

    N, S, M, H = 4, 16, 3, 6
    g = torch.Generator().manual_seed(3)
    mu = 0.4 * torch.randn(N, H, 1, generator=g)
    th = mu + 0.6 * torch.randn(N, H, 1, generator=g)
    cov = 4.0 * torch.eye(1)
    model = PendulumModel(uncertain_params=("length", "mass"))
    cost = PendulumQuadCos()
    ctrl = MultiDISCO(model.observation_space, model.action_space, H, N, S, temperature=1.0, a_cov=cov, inst_cost_fn=cost.inst_cost,
                      term_cost_fn=cost.term_cost, params_sampling=True, params_samples=M, seed=40)
    ctrl.a_mat = th.clone()
    ctrl.return_rollouts = False
    mpf = MPF(init_particles=x0[envs[0]].clone(), likelihood=GaussianLikelihood(initial_obs=states[envs[0]], obs_std=0.2, model=model, log_space=False),
              optimizer_class=torch.optim.SGD, lr=1e-6, bw=0.05)
    kw = dict(init_particles=th.clone(), prior=get_gmm(mu, torch.ones(N), cov), kernel=RBFKernel(), n_particles=N, n_steps=2,
              likelihood=ExponentiatedUtility(alpha=1.0, n_samples=S, controller=ctrl, model=model), optimizer_class=torch.optim.SGD, lr=0.5)
    return BatchDualSVMPC(BatchSVMPC(len(envs), seeds=[40 + e for e in envs], **kw), mpf, mpf_bw=mpf_bw, mpf_steps=sw.MPF_STEPS,
                          seed=seed + (envs[0] << 32 if len(envs) == 1 else 0), init_particles=x0[envs])


def test_class_with_filter_rows_against_one_environment_objects():
    """BatchDualSVMPC.set_filter_hyper (B = 3) against three one-environment objects holding one row each, three periods under one
    prescribed sequence of states and actions, bit for bit; a deep copy taken after the first period carries the rows and continues"""
    B, seed, Mp = 3, 20260, 48
    g = torch.Generator().manual_seed(5)
    x0 = torch.tensor([1.0, 1.0]) * (1.0 + 0.05 * torch.randn(B, Mp, 2, generator=g))
    states = torch.tensor([3.0, 0.0])[None] + 0.01 * torch.randn(B, 2, generator=g)
    p = dict(lr=sw.f32(1e-6), obs_std=sw.f32(0.2), bw=0.0, bw_scale=1.0)
    rows = [dict(p, lr=sw.f32(4e-6)), dict(p, bw=sw.f32(0.05)), dict(p, obs_std=sw.f32(0.1), bw_scale=0.5)]
    loop = _loop(B, seed, [0, 1, 2], x0, states)
    assert _hyper_list(loop.filter_hyper) == [p] * B
    loop.set_filter_hyper([{k: r[k] for k in r if r[k] != p[k]} for r in rows])  # (fields left out: the prototype's)
    assert _hyper_list(loop.filter_hyper) == rows
    ones = [_loop(1, seed, [b], x0, states) for b in range(B)]
    for b, o in enumerate(ones):
        o.set_filter_hyper([rows[b]])
    twin = None
    rng = np.random.default_rng(4)
    for t in range(3):
        if t > 0:
            actions = torch.from_numpy((0.3 * rng.standard_normal((B, 1))).astype(np.float32))
            states = states + torch.from_numpy((0.02 * rng.standard_normal(tuple(states.shape))).astype(np.float32))
            for o in [loop] + ([twin] if twin is not None else []):
                o.step(actions, states)
            for b, o in enumerate(ones):
                o.step(actions[b:b + 1], states[b:b + 1])
        a_b, pw_b = loop.forward(states)
        if twin is not None:
            a_t, pw_t = twin.forward(states)
            assert torch.equal(a_t, a_b) and torch.equal(pw_t, pw_b) and torch.equal(twin.dyn_particles, loop.dyn_particles), t
            assert torch.equal(twin.last_bw, loop.last_bw)
        x = loop.dyn_particles
        for b, o in enumerate(ones):
            a_1, pw_1 = o.forward(states[b:b + 1])
            assert torch.equal(a_1[0], a_b[b]) and torch.equal(pw_1[0], pw_b[b]), (t, b)
            assert torch.equal(o.dyn_particles[0], x[b]), (t, b)
            if t > 0:
                assert float(o.last_bw[0]) == float(loop.last_bw[b]), (t, b)
        if t > 0:
            assert float(loop.last_bw[1]) == np.float32(0.05) and float(loop.last_bw[0]) != float(loop.last_bw[2])
        if t == 0:
            twin = copy.deepcopy(loop)
            assert twin._mb is not loop._mb and _hyper_list(twin.filter_hyper) == rows
    loop.set_filter_hyper(None)
    assert _hyper_list(loop.filter_hyper) == [p] * B and _hyper_list(twin.filter_hyper) == rows


def _pendulum_driver_args(B, Mp=16):
    from dust_amd.controllers import MultiDISCO
    from dust_amd.costs import PendulumQuadCos
    from dust_amd.inference import MPF, GaussianLikelihood, get_gmm
    from dust_amd.kernels import RBFKernel
    from dust_amd.models import PendulumModel

    N, S, M, H = 3, 16, 3, 6
    g = torch.Generator().manual_seed(11)
    model_kwargs = dict(uncertain_params=("length", "mass"))
    model = PendulumModel(**model_kwargs)
    cost = PendulumQuadCos()
    cov = 4.0 * torch.eye(1)
    ctrl = MultiDISCO(model.observation_space, model.action_space, H, N, S, temperature=1.0, a_cov=cov, inst_cost_fn=cost.inst_cost,
                      term_cost_fn=cost.term_cost, params_sampling=True, params_samples=M, seed=1)
    mu = 0.4 * torch.randn(N, H, 1, generator=g)
    th = mu + 0.6 * torch.randn(N, H, 1, generator=g)
    state = torch.tensor([3.0, 0.0])
    x0 = torch.tensor([1.0, 1.0]) * (1.0 + 0.1 * torch.randn(Mp, 2, generator=g))
    mpf = MPF(init_particles=x0, likelihood=GaussianLikelihood(initial_obs=state, obs_std=0.2, model=model, log_space=False),
              optimizer_class=torch.optim.SGD, lr=1e-5, bw=0.05)
    svmpc_kwargs = dict(init_particles=th.clone(), prior=get_gmm(mu, torch.ones(N), cov), kernel=RBFKernel(), n_particles=N, n_steps=2,
                        optimizer_class=torch.optim.SGD, lr=0.5, seeds=list(range(50, 50 + B)))
    lik_kwargs = dict(alpha=1.0, n_samples=S)
    exp = [dict(length=0.8 + 0.05 * b, mass=1.25) for b in range(B)]
    return dict(init_state=state, init_policies=th, model_kwargs=model_kwargs, experiment_params=exp, controller=ctrl, svmpc_kwargs=svmpc_kwargs,
                lik_kwargs=lik_kwargs, mpf=mpf), model


def test_pendulum_driver_takes_the_rows():
    """run_pendulum_simulations(mpf_hyper=) against BatchDualSVMPC.simulate called directly with the rows set, and against the same run
    without rows (which must differ); a positive mpf_bw beside rows is refused before any device call"""
    from dust_amd.controllers.dual import BatchDualSVMPC
    from dust_amd.inference import BatchSVMPC, ExponentiatedUtility
    from dust_amd.utils.simulations import run_pendulum_simulations

    B, steps = 3, 4
    args, model = _pendulum_driver_args(B)
    p = dict(lr=sw.f32(1e-5), obs_std=sw.f32(0.2), bw=0.0, bw_scale=1.0)
    rows = [dict(lr=sw.f32(4e-5)), dict(bw=sw.f32(0.05)), dict(obs_std=sw.f32(0.1), bw_scale=0.5)]
    out = run_pendulum_simulations(**args, mpf_steps=sw.MPF_STEPS, episodes=B, steps=steps, warm_up=1, seed=9, mpf_hyper=rows)
    plain = run_pendulum_simulations(**args, mpf_steps=sw.MPF_STEPS, episodes=B, steps=steps, warm_up=1, seed=9)
    assert not np.array_equal(out["DynParticles"], plain["DynParticles"])
    assert (out["DynBandwidths"][1, 1:] == np.float32(0.05)).all()
    ctrl = copy.deepcopy(args["controller"])
    ctrl.a_mat = args["init_policies"].detach().clone()
    ctrl.return_rollouts = False
    sv = BatchSVMPC(B, likelihood=ExponentiatedUtility(**args["lik_kwargs"], controller=ctrl, model=model), **args["svmpc_kwargs"])
    dual = BatchDualSVMPC(sv, args["mpf"], mpf_steps=sw.MPF_STEPS, seed=9, warm_up=1)
    dual.set_filter_hyper(rows)
    assert _hyper_list(dual.filter_hyper) == [dict(p, **r) for r in rows]
    true = torch.tensor([[e["length"], e["mass"]] for e in args["experiment_params"]], dtype=torch.float)
    res = dual.simulate(args["init_state"].reshape(1, -1).repeat(B, 1), steps, plant_params=true)
    assert np.array_equal(res.bw.transpose(0, 1).numpy(), out["DynBandwidths"])
    assert np.array_equal(res.actions.transpose(0, 1).numpy().reshape(B, steps), out["Actions"].reshape(B, steps))
    assert np.array_equal(dual.dyn_particles.numpy(), out["DynParticles"])
    with pytest.raises(ValueError, match="put it in the rows"):
        run_pendulum_simulations(**args, mpf_bw=0.05, mpf_steps=sw.MPF_STEPS, episodes=B, steps=steps, warm_up=1, seed=9, mpf_hyper=rows)


def test_the_example_runs():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "pendulum_filter_sweep_example.py"), "--tiny"], capture_output=True, text=True,
                         timeout=300, env=dict(os.environ, PYTHONPATH=ROOT))
    assert out.returncode == 0, out.stderr[-2000:]
    assert "best rows" in out.stdout and "AvgCumCost" in out.stdout, out.stdout[-2000:]
