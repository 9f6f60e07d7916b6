"""The posterior's history out of the device episodes (dust_svmpc_batch_set_history / dust_svmpc_batch_get_history; csrc/svmpc_episode.hpp
svmpc_sim_hist_kernel and svmpc_dual_sim_hist_period_kernel; `SvmpcBatch.set_history` / `history`, `BatchSVMPC.history`,
`BatchDualSVMPC.history`, `run_pendulum_simulations(history=True)`).  Every comparison below is np.array_equal - bit for bit; the cases and
why each exists are in tests/svmpc_history_cases.py.

1. a recording call against its periods on clones taken before it (the per-period loops of test_gpu_svmpc_sim.py and
   test_gpu_svmpc_dual_sim.py, fed the recorded states, the host applying the rules through the imported fp32 replicas): theta_hist[t, b]
   is the clone's DUST_SVB_THETA after per-period call t, x_hist[t, b] the clone filters' particles after per-period dual call t, for
   every period each environment ran;
2. every other row still holds the sentinel the test put there;
3. recording changes nothing else: the same call on a clone with recording off - every output, every getter, the filters, one further call;
4. the launch counts with recording on and off, the filter side's independent of B;
5. two chained calls against one; 6. an environment records the same alone, in slots 0 / 2 / 4 of five, beside inactive, already
   stopped and earlier-stopping neighbours; 7. what get_history answers when; 8. refusals; 9. the classes, the driver, the example.
"""
import copy
import ctypes as C
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import svmpc_episode_cases as ec
import svmpc_history_cases as cases
import svmpc_sim_cases as sc
import test_gpu_svmpc_dual_sim as ds
import test_gpu_svmpc_sim as ps
from test_gpu_svmpc_dual_episode import GETTERS, ROOT, _setup, _state

pytestmark = pytest.mark.gpu

SENT = np.float32(7.5)  # what the tests fill an output with: a row the library did not write still holds it


@pytest.fixture(autouse=True)
def _single_workgroup_filters(monkeypatch):
    """(the switch is read in dust_mpf_create; the batched filter kernels do not depend on it)"""
    monkeypatch.setenv("DUST_MPF_GRID", "0")


def _L():
    from dust_amd import _lib

    return _lib


def _get(sb, which, row=None, fill=SENT):
    """dust_svmpc_batch_get_history through the raw binding into an array filled with `fill` -> (status, T, array or None)"""
    L = _L()
    lib, T = L.load(), C.c_int(-1)
    code = lib.dust_svmpc_batch_get_history(sb._h, int(which), C.byref(T), None)
    if code != L.OK or row is None:
        return code, T.value, None
    out = np.full((T.value, sb.B) + tuple(row), fill, np.float32)
    assert lib.dust_svmpc_batch_get_history(sb._h, int(which), None, out.ctypes.data_as(L.FP)) == L.OK
    return code, T.value, out


def _theta_hist(sb):
    code, T, out = _get(sb, _L().HIST_THETA, (sb.N, sb.H, sb.da))
    assert code == _L().OK
    return out


def _x_hist(sb, mb):
    code, T, out = _get(sb, _L().HIST_FILTER, (mb.Mp, mb.P))
    assert code == _L().OK
    return out


def _eq(u, v):
    return (u is None and v is None) or np.array_equal(u, v, equal_nan=True)


def _same_state(x, y, fwd=None):
    """two pairs show the same of themselves; fwd [B]: the environments that ran a forward() (log_p is written by forward() alone)"""
    assert set(x) == set(y)
    for n in x:
        if n == "LOG_P" and fwd is not None:
            assert np.array_equal(x[n][fwd], y[n][fwd]), n
        else:
            assert np.array_equal(x[n], y[n]), n


# ------------------------------------------------------------------------------------------------ the plain call
def _plain_call(case, b, inp, envs=None, T=None, t0=0, T0=0, st=None, loss=None, status=None, active=None):
    envs = list(range(case["B"])) if envs is None else list(envs)
    T = case["T"] if T is None else T
    st0, params, plant = ps._sub(inp, envs, T0, T0 + T)
    return b.simulate(st0 if st is None else st, T, case["n_steps"], params, plant, t0=t0, loss=loss, status=status, active=active, **ps._rules(case))


@functools.lru_cache(maxsize=None)
def _plain(cid):
    """the case's recording call; on a clone taken before it, its periods - optimize while warming up, the tick afterwards - fed the
    recorded states, theta read after every one; on another clone the same call with recording off; one further tick on all three"""
    L = _L()
    case = cases.PLAIN_BY_ID[cid]
    T, B, n, grid, warm = case["T"], case["B"], case["n_steps"], sc.grid_of(case), case["rules"]["warm_up"]
    inp = ps._inputs(case)
    b = ps._batch(case, inp)
    twin, off = b.clone(), b.clone()
    b.set_history(theta=True)
    out = _plain_call(case, b, inp)
    hist = _theta_hist(b)
    out_off = _plain_call(case, off, inp)
    st, params, _ = ps._sub(inp, range(B), 0, T)
    xs = out[0]
    on, status, n_run = np.ones(B, bool), np.zeros(B, np.int32), np.zeros(B, np.int32)
    x, periods = st.copy(), []
    for t in range(T):
        if not on.any():
            break
        prm = None if params is None else params[t]
        if t < warm:
            twin.optimize(x, n, params=prm, active=on)
        else:
            twin.tick(x, n, params=prm, active=on)
        periods.append((t, on.copy(), twin.get(L.SVB_THETA)))
        x[on] = xs[t][on]
        n_run[on] += 1
        status[on] = sc.apply_rules(case, xs[t][on], grid)
        on &= status == 0
    res = dict(inp=inp, out=out, out_off=out_off, hist=hist, periods=periods, n_run=n_run, after=(ps._records(b), ps._records(twin), ps._records(off)))
    extra = None if inp["params"] is None else inp["params"][T]
    x = np.nan_to_num(x)
    res["further"] = [h.tick(x, n, params=extra) for h in (b, twin, off)]
    res["after_further"] = (ps._records(b), ps._records(off))
    res["hist_after_tick"] = _theta_hist(b)  # (a non-recording call leaves the recording in place)
    for h in (b, twin, off):
        h.close()
    return res


@pytest.mark.parametrize("cid", cases.PLAIN_IDS)
def test_plain_history_equals_the_per_period_calls(cid):
    case, r = cases.PLAIN_BY_ID[cid], _plain(cid)
    T, B, f = case["T"], case["B"], ec.family(case)
    hist, n_run = r["hist"], r["out"][6]
    assert hist.shape == (T, B, case["N"], case["H"], f["da"])
    assert np.array_equal(n_run, r["n_run"])
    print(cid, "n_run", n_run.tolist())
    seen = np.zeros((T, B), bool)
    for t, on, theta in r["periods"]:
        assert np.array_equal(on, n_run > t), t
        assert np.array_equal(hist[t][on], theta[on]), (cid, t)
        assert np.isfinite(hist[t][on]).all()
        seen[t] = on
    assert seen.sum() == n_run.sum()
    assert (hist[~seen] == SENT).all()  # 2. rows at or past n_run[b]: not written
    assert (hist[seen] != SENT).any()
    for e, (period, _) in cases.DUAL_EVENTS.get(cid, {}).items():
        assert n_run[e] == period + 1
    if T > 1 and n_run.max() > 1:  # successive rows differ: a row is its own period's
        e = int(np.argmax(n_run))
        assert not np.array_equal(hist[0, e], hist[1, e])
    assert np.array_equal(r["hist_after_tick"], hist)


@pytest.mark.parametrize("cid", cases.PLAIN_IDS)
def test_plain_recording_changes_nothing_else(cid):
    case, r = cases.PLAIN_BY_ID[cid], _plain(cid)
    for k, (u, v) in enumerate(zip(r["out"], r["out_off"])):  # states, actions, weights, costs, loss, status, n_run, a_seq
        assert _eq(u, v), k
    fwd = r["out"][6] > case["rules"]["warm_up"]
    ps._same(r["after"][0], r["after"][2], fwd=fwd)
    ps._same(r["after"][0], r["after"][1], fwd=fwd)
    (a1, p1), (a2, p2), (a3, p3) = r["further"]
    assert np.array_equal(a1, a3) and np.array_equal(p1, p3) and np.array_equal(a1, a2) and np.array_equal(p1, p2)
    ps._same(*r["after_further"])


# ------------------------------------------------------------------------------------------------ the dual call
def _dual_periods(case, sb, mb, st, ap, seeds, T, xs, on=None, t0=0):
    """test_gpu_svmpc_dual_sim._periods, reading theta and the filters' particles after every per-period call:
    -> ([(on, theta, x)], n_run, status)"""
    L = _L()
    grid = ds.cases.grid_of(case)
    B = len(st)
    on = np.ones(B, bool) if on is None else np.array(on, bool)
    n_run, status = np.zeros(B, np.int32), np.zeros(B, np.int32)
    x = np.array(st, np.float32)
    a = None if ap is None else np.array(ap, np.float32)
    out = []
    for t in range(T):
        a_t, _, _ = ds._period(case, sb, mb, t0 + t, x, a, seeds[t], active=on.astype(np.uint8))
        out.append((on.copy(), sb.get(L.SVB_THETA), mb.get_particles()))
        a = np.where(on[:, None], a_t, np.zeros_like(a_t) if a is None else a)
        x = np.where(on[:, None], np.nan_to_num(xs[t]), x)
        n_run[on] += 1
        status[on] = sc.apply_rules(case, x, grid)[on]
        on &= status == 0
    return out, n_run, status


@functools.lru_cache(maxsize=None)
def _dual(cid):
    """the case's recording call (theta and filter), its periods on clones of both batches taken before it, and the same call on another
    pair of clones with recording off; then one further dual tick on the recording pair and on the pair that did not record"""
    case = cases.DUAL_BY_ID[cid]
    T = case["T"]
    st, ap, rows, seeds = ds._inputs(case)
    sb, mb = _setup(case)
    before = mb.get_particles()
    sb2, mb2 = sb.clone(), mb.clone()
    sb3, mb3 = sb.clone(), mb.clone()
    sb.set_history(theta=True, filter=True)
    s0, s03 = mb.stats(), mb3.stats()
    out = ds._sim(case, sb, mb, st, ap, rows, seeds, T)
    th, xh = _theta_hist(sb), _x_hist(sb, mb)
    out_off = ds._sim(case, sb3, mb3, st, ap, rows, seeds, T)
    s1, s13 = mb.stats(), mb3.stats()
    periods, n_run, status = _dual_periods(case, sb2, mb2, st, ap, seeds, T, out[0])
    names = GETTERS if case["rules"]["warm_up"] < T else ds.OPT_GETTERS
    r = dict(st=st, ap=ap, rows=rows, seeds=seeds, out=out, out_off=out_off, th=th, xh=xh, periods=periods, n_run=n_run, before=before,
             after=(_state(sb, mb, names), _state(sb2, mb2, names), _state(sb3, mb3, names)),
             stats=({k: s1[k] - s0[k] for k in s0}, {k: s13[k] - s03[k] for k in s03}))
    pend = ds._pending(st, ap, out)
    r["further"] = (ds._further(case, sb, mb, pend, seeds[T]), ds._further(case, sb3, mb3, pend, seeds[T]), _state(sb, mb), _state(sb3, mb3))
    r["hist_after_tick"] = (_theta_hist(sb), _x_hist(sb, mb))
    for h in (sb, mb, sb2, mb2, sb3, mb3):
        h.close()
    return r


@pytest.mark.parametrize("cid", cases.DUAL_IDS)
def test_dual_history_equals_the_per_period_calls(cid):
    case, r = cases.DUAL_BY_ID[cid], _dual(cid)
    T, B, f = case["T"], case["B"], ec.family(case)
    th, xh, n_run = r["th"], r["xh"], r["out"][7]
    assert th.shape == (T, B, case["N"], case["H"], f["da"]) and xh.shape == (T, B, case["Mp"], len(case["up"]))
    assert np.array_equal(n_run, r["n_run"])
    print(cid, "n_run", n_run.tolist())
    seen = np.zeros((T, B), bool)
    for t, (on, theta, x) in enumerate(r["periods"]):
        assert np.array_equal(on, n_run > t), t
        assert np.array_equal(th[t][on], theta[on]), (cid, t)
        assert np.array_equal(xh[t][on], x[on]), (cid, t)
        assert np.isfinite(th[t][on]).all() and np.isfinite(xh[t][on]).all()
        seen[t] = on
    assert (th[~seen] == SENT).all() and (xh[~seen] == SENT).all()  # 2. rows at or past n_run[b]: not written
    for e, (period, _) in cases.DUAL_EVENTS.get(cid, {}).items():
        assert n_run[e] == period + 1
    # row 0: the particles at entry without actions_prev, behind an update with it
    ran = n_run > 0
    if case["first"]:
        assert all(not np.array_equal(xh[0, e], r["before"][e]) for e in np.nonzero(ran)[0])
    else:
        assert np.array_equal(xh[0][ran], r["before"][ran])
    if T > 1:  # later rows lie behind updates (the Particle filter moves only behind a tick's action: svmpc_dual_sim_cases)
        e = int(np.argmax(n_run))
        assert not np.array_equal(th[0, e], th[1, e])
        if case["family"] == "pendulum":
            assert not np.array_equal(xh[0, e], xh[1, e])
    assert np.array_equal(r["hist_after_tick"][0], th) and np.array_equal(r["hist_after_tick"][1], xh)


@pytest.mark.parametrize("cid", cases.DUAL_IDS)
def test_dual_recording_changes_nothing_else(cid):
    case, r = cases.DUAL_BY_ID[cid], _dual(cid)
    for k, (u, v) in enumerate(zip(r["out"], r["out_off"])):  # xs, acts, pw, bw, costs, loss, status, n_run, a_seq
        assert _eq(u, v), k
    fwd = r["out"][7] > case["rules"]["warm_up"]
    _same_state(r["after"][0], r["after"][2], fwd)
    _same_state(r["after"][0], r["after"][1], fwd)
    assert r["stats"][0] == r["stats"][1] and r["stats"][0]["calls"] == case["T"]
    (a1, p1, b1), (a3, p3, b3), g1, g3 = r["further"]
    assert np.array_equal(a1, a3) and np.array_equal(p1, p3) and np.array_equal(b1, b3)
    _same_state(g1, g3)


# ------------------------------------------------------------------------------------------------ 4. launch counts
def _dual_launches(case, envs, record):
    st, ap, rows, seeds = ds._inputs(case, envs)
    sb, mb = _setup(case, envs)
    if record:
        sb.set_history(theta=True, filter=True)
    sb.ctx.profile(True)
    s0 = mb.stats()
    ds._sim(case, sb, mb, st, ap, rows, seeds, case["T"])
    prof = {k: v[1] for k, v in sb.ctx.profile_get().items() if v[1]}
    s1 = mb.stats()
    sb.close()
    mb.close()
    return prof, s1["launches"] - s0["launches"]


def test_launch_counts_do_not_change():
    case = cases.DUAL_BY_ID["P1"]  # Silverman's rule: two filter launches per period that has an update
    T = case["T"]
    on, off = _dual_launches(case, [0, 1, 2], True), _dual_launches(case, [0, 1, 2], False)
    assert on == off and on[0] == {"svmpc_batch_kernel": T} and on[1] == 2 * (T - 1)
    assert _dual_launches(case, [1], True) == on == _dual_launches(case, [0, 1, 2, 1, 0, 2, 1], True)  # ... whatever B
    # the plain call: one launch
    pc = cases.PLAIN_BY_ID["P1"]
    inp = ps._inputs(pc)
    counts = []
    for record in (True, False):
        b = ps._batch(pc, inp)
        if record:
            b.set_history(theta=True)
        b.ctx.profile(True)
        _plain_call(pc, b, inp)
        counts.append({k: v[1] for k, v in b.ctx.profile_get().items() if v[1]})
        b.close()
    assert counts[0] == counts[1] == {"svmpc_batch_kernel": 1}


# ------------------------------------------------------------------------------------------------ 5. chaining
@pytest.mark.parametrize("cid", ["P1", "P3"])
def test_two_chained_dual_calls_record_what_one_records(cid):
    """split inside the warm-up (P1: 1 of 2) and after it (P1: 3); P3: behind the period that stops two environments"""
    case, r = cases.DUAL_BY_ID[cid], _dual(cid)
    T = case["T"]
    for T1 in ((1, 3) if cid == "P1" else (1, 2)):
        sb, mb = _setup(case)
        sb.set_history(theta=True, filter=True)
        one = ds._sim(case, sb, mb, r["st"], r["ap"], r["rows"], r["seeds"][:T1])
        th1, xh1 = _theta_hist(sb), _x_hist(sb, mb)
        a1, x1 = ds._pending(r["st"], r["ap"], one)
        two = ds._sim(case, sb, mb, x1, a1, r["rows"], r["seeds"][T1:T], t0=T1, loss=one[5], status=one[6])
        th2, xh2 = _theta_hist(sb), _x_hist(sb, mb)
        sb.close()
        mb.close()
        assert len(th1) == len(xh1) == T1 and len(th2) == len(xh2) == T - T1
        assert np.array_equal(np.concatenate((th1, th2)), r["th"]), T1
        assert np.array_equal(np.concatenate((xh1, xh2)), r["xh"]), T1
        assert np.array_equal(one[7] + two[7], r["out"][7])


def test_two_chained_plain_calls_record_what_one_records():
    case, r = cases.PLAIN_BY_ID["P1"], _plain("P1")
    T, inp = case["T"], r["inp"]
    for T1 in (1, 3):  # inside the warm-up of 2, and after it
        b = ps._batch(case, inp)
        b.set_history(theta=True)
        one = _plain_call(case, b, inp, T=T1)
        h1 = _theta_hist(b)
        two = _plain_call(case, b, inp, T=T - T1, t0=T1, T0=T1, st=one[0][-1], loss=one[4], status=one[5])
        h2 = _theta_hist(b)
        b.close()
        assert len(h1) == T1 and len(h2) == T - T1 and np.array_equal(np.concatenate((h1, h2)), r["hist"]), T1
        assert np.array_equal(np.concatenate((one[0], two[0])), r["out"][0])


# ------------------------------------------------------------------------------------------------ 6. isolation
@pytest.mark.parametrize("cid,e", [("P1", 2), ("P3", 2)])
def test_an_environment_records_the_same_in_any_batch(cid, e):
    """alone; in slots 0 / 2 / 4 of five; beside inactive and already-stopped neighbours; P3: its own batch's neighbours 0 and 1 stop in
    period 0 (the full run)"""
    case, r = cases.DUAL_BY_ID[cid], _dual(cid)
    T = case["T"]
    want_th, want_x = r["th"][:, e], r["xh"][:, e]
    assert r["out"][7][e] == T

    def run(envs, **kw):
        st, ap, rows, seeds = ds._inputs(case, envs)
        sb, mb = _setup(case, envs)
        sb.set_history(theta=True, filter=True)
        out = ds._sim(case, sb, mb, st, ap, rows, seeds, T, **kw)
        got = _theta_hist(sb), _x_hist(sb, mb), out
        sb.close()
        mb.close()
        return got

    th, xh, _ = run([e])
    assert np.array_equal(th[:, 0], want_th) and np.array_equal(xh[:, 0], want_x)
    th, xh, _ = run([e, 0, e, 1, e])
    for slot in (0, 2, 4):
        assert np.array_equal(th[:, slot], want_th) and np.array_equal(xh[:, slot], want_x), slot
    for kw in (dict(active=[0, 1, 0]), dict(status=np.array([2, 0, 1], np.int32), loss=np.array([np.inf, 0, 3.5], np.float32))):
        th, xh, out = run([0, e, 1], **kw)
        assert np.array_equal(th[:, 1], want_th) and np.array_equal(xh[:, 1], want_x), sorted(kw)
        assert (th[:, [0, 2]] == SENT).all() and (xh[:, [0, 2]] == SENT).all(), sorted(kw)  # 2. nothing of them is written
        assert out[7][1] == T


def test_a_plain_environment_records_the_same_beside_inactive_and_stopped_neighbours():
    case, r = cases.PLAIN_BY_ID["P3"], _plain("P3")
    e, T, inp = 2, case["T"], r["inp"]
    assert r["out"][6][e] == T
    for envs, kw in (([e], {}), ([0, e, 1], dict(active=np.array([0, 1, 0], np.uint8))),
                     ([0, e, 1], dict(status=np.array([2, 0, 1], np.int32), loss=np.array([np.inf, 0, 3.5], np.float32)))):
        b = ps._batch(case, inp, envs)
        b.set_history(theta=True)
        _plain_call(case, b, inp, envs, **kw)
        h = _theta_hist(b)
        b.close()
        slot = envs.index(e)
        assert np.array_equal(h[:, slot], r["hist"][:, e]), sorted(kw)
        others = [k for k in range(len(envs)) if k != slot]
        assert (h[:, others] == SENT).all(), sorted(kw)


# ------------------------------------------------------------------------------------------------ 7. get_history
def test_what_get_history_answers_when():
    L = _L()
    lib = L.load()
    case = cases.DUAL_BY_ID["P1"]
    T = case["T"]
    st, ap, rows, seeds = ds._inputs(case)
    sb, mb = _setup(case)
    for which in (L.HIST_THETA, L.HIST_FILTER):  # before any recording - with the setting off and on
        assert _get(sb, which)[0] == L.ERR_STATE
    sb.set_history(theta=True, filter=True)
    for which in (L.HIST_THETA, L.HIST_FILTER):
        assert _get(sb, which)[0] == L.ERR_STATE
    assert lib.dust_svmpc_batch_get_history(sb._h, 0, None, None) == L.ERR_INVALID
    assert lib.dust_svmpc_batch_get_history(sb._h, 3, None, None) == L.ERR_INVALID
    assert lib.dust_svmpc_batch_get_history(None, L.HIST_THETA, None, None) == L.ERR_INVALID
    # a non-rule episode ignores the setting: it records nothing
    pair = sb.clone(), mb.clone()
    pair[0].dual_episode(pair[1], st, 2, case["n_steps"], ap, mpf_steps=case["mpf_steps"], mpf_bw=case["mpf_bw"], seeds=seeds[:2], plant_params=rows)
    assert _get(pair[0], L.HIST_THETA)[0] == L.ERR_STATE and _get(pair[0], L.HIST_FILTER)[0] == L.ERR_STATE
    for h in pair:
        h.close()
    out = ds._sim(case, sb, mb, st, ap, rows, seeds, T)
    assert _get(sb, L.HIST_THETA)[:2] == (L.OK, T) and _get(sb, L.HIST_FILTER)[:2] == (L.OK, T)  # n_periods with a NULL out
    th, xh = _theta_hist(sb), _x_hist(sb, mb)
    # the class's accessor: NaN where the raw call leaves the caller's fill
    assert np.array_equal(sb.history(L.HIST_THETA), np.where(th == SENT, np.nan, th), equal_nan=True)
    assert np.array_equal(sb.history(L.HIST_FILTER), np.where(xh == SENT, np.nan, xh), equal_nan=True)
    # a clone carries the setting and has no rows
    twin_sb, twin_mb = sb.clone(), mb.clone()
    assert _get(twin_sb, L.HIST_THETA)[0] == L.ERR_STATE and _get(twin_sb, L.HIST_FILTER)[0] == L.ERR_STATE
    a, x = ds._pending(st, ap, out)
    more = ds._sim(case, twin_sb, twin_mb, x, a, rows, seeds[:2], t0=T, loss=out[5], status=out[6])
    assert _get(twin_sb, L.HIST_THETA)[:2] == (L.OK, 2) and (more[7] == 2).all()
    # non-recording calls leave the last recording in place: a plain tick, a dual tick
    sb.tick(x, case["n_steps"], params=ec.tick_params(case, 1)[0])
    ds._further(case, sb, mb, (a, x), seeds[T])
    assert np.array_equal(_theta_hist(sb), th) and np.array_equal(_x_hist(sb, mb), xh)
    # theta alone: the filter's last recording stays; the plain call records theta, and nothing with the filter bit alone
    sb.set_history(theta=False, filter=True)
    inp = ps._inputs(cases.PLAIN_BY_ID["P1"])
    _plain_call(cases.PLAIN_BY_ID["P1"], sb, inp, T=2)
    assert np.array_equal(_theta_hist(sb), th) and np.array_equal(_x_hist(sb, mb), xh)
    sb.set_history(theta=True, filter=False)
    _plain_call(cases.PLAIN_BY_ID["P1"], sb, inp, T=2)
    assert _get(sb, L.HIST_THETA)[:2] == (L.OK, 2) and np.array_equal(_x_hist(sb, mb), xh)
    # off: the recordings go
    sb.set_history()
    assert _get(sb, L.HIST_THETA)[0] == L.ERR_STATE and _get(sb, L.HIST_FILTER)[0] == L.ERR_STATE
    with pytest.raises(L.DustError) as err:
        sb.history(L.HIST_THETA)
    assert err.value.status == L.ERR_STATE
    for h in (sb, mb, twin_sb, twin_mb):
        h.close()


# ------------------------------------------------------------------------------------------------ 8. refusals
def _refused(b, case, inp, st, T, n, words):
    """a raw simulate call that must be refused as unsupported: no launch, nothing written, the message names the way out"""
    L = _L()
    total = lambda: sum(v[1] for v in b.ctx.profile_get().values())
    before = ps._records(b)
    loss, status = np.full(b.B, 1.5, np.float32), np.zeros(b.B, np.int32)
    got = ps._raw(b, case, inp, st, T, n, fill=7.5, loss=loss, status=status)
    assert got["code"] == L.ERR_UNSUPPORTED, got["code"]
    msg = L.load().dust_last_error().decode()
    assert words in msg, msg
    assert total() == 0
    for a in got["arrays"]:
        assert (a == 7.5).all()
    assert (got["loss"] == 1.5).all() and not got["status"].any() and (got["n_run"] == -1).all()
    ps._same(ps._records(b), before)
    return msg


def test_refusals_come_before_anything_is_allocated_staged_or_launched():
    L = _L()
    lib = L.load()
    # unknown bits
    case = sc.BY_ID["pend_rows"]
    inp = ps._inputs(case)
    b = ps._batch(case, inp)  # (with its per-environment controller rows)
    for bad in (4, 7, -1, 1 << 30):
        assert lib.dust_svmpc_batch_set_history(b._h, bad) == L.ERR_INVALID
    assert lib.dust_svmpc_batch_set_history(None, 1) == L.ERR_INVALID
    # controller rows set
    st, _, _ = ps._sub(inp, range(case["B"]), 0, case["T"])
    b.simulate(st, 1, case["n_steps"], inp["params"][:1], inp["plant"], **ps._rules(case))  # (so that every getter has something to keep)
    b.ctx.profile(True)
    b.set_history(theta=True)
    _refused(b, case, inp, st, case["T"], case["n_steps"], "dust_svmpc_batch_set_history(batch, 0)")
    assert _get(b, L.HIST_THETA)[0] == L.ERR_STATE
    b.set_history(theta=False, filter=True)  # the plain call records nothing under the filter bit alone: the sweep instance runs
    assert ps._raw(b, case, inp, st, case["T"], case["n_steps"])["code"] == L.OK
    b.set_history()
    assert ps._raw(b, case, inp, st, case["T"], case["n_steps"])["code"] == L.OK
    b.close()
    # a navigation-cost prototype
    case = sc.BY_ID["skid_nav"]
    inp = ps._inputs(case)
    b = ps._batch(case, inp)
    st, _, _ = ps._sub(inp, range(case["B"]), 0, case["T"])
    b.simulate(st, 1, case["n_steps"], inp["params"][:1], inp["plant"], **ps._rules(case))
    b.ctx.profile(True)
    b.set_history(theta=True)
    _refused(b, case, inp, st, case["T"], case["n_steps"], "dust_svmpc_batch_set_history(batch, 0)")
    b.set_history()
    assert ps._raw(b, case, inp, st, case["T"], case["n_steps"])["code"] == L.OK
    b.close()
    # the size cap: N 64, D 128, T 4096, B 9 - nothing of that size is ever allocated
    case = cases.PLAIN_BY_ID["P6"]
    cap = cases.CAP
    assert (case["N"], case["H"]) == (cap["N"], cap["H"])
    inp = ps._inputs(case)
    envs = [k % case["B"] for k in range(cap["B"])]
    b = ps._batch(case, inp, envs)
    st = inp["st"][envs]
    sub = dict(inp, plant=None, params=None)
    b.simulate(st, 1, case["n_steps"], None, None, **ps._rules(case))
    b.ctx.profile(True)
    b.set_history(theta=True)
    msg = _refused(b, case, sub, st, cap["T"], case["n_steps"], "split the episode")
    assert str(cap["T"] * cap["B"] * cap["N"] * cap["H"] * 2) in msg
    assert _get(b, L.HIST_THETA)[0] == L.ERR_STATE
    assert ps._raw(b, case, sub, st, 2, case["n_steps"])["code"] == L.OK  # a shorter call records
    assert _get(b, L.HIST_THETA)[:2] == (L.OK, 2)
    b.close()


def test_filter_rows_keep_working_under_recording():
    """per-environment FILTER rows touch the filter's kernels alone: accepted, and environment b records what a one-environment pair
    built with row b records"""
    case = cases.DUAL_BY_ID["P1"]  # (Silverman's rule: the rows may carry bandwidth scales)
    T = case["T"]
    hyper = [dict(lr=1e-3), dict(lr=2e-3, obs_std=0.3), dict(bw_scale=0.5)]
    st, ap, rows, seeds = ds._inputs(case)
    sb, mb = _setup(case)
    mb.set_hyper(hyper)
    sb.set_history(theta=True, filter=True)
    out = ds._sim(case, sb, mb, st, ap, rows, seeds, T)
    th, xh = _theta_hist(sb), _x_hist(sb, mb)
    sb.close()
    mb.close()
    assert (out[7] == T).all() and not np.array_equal(xh, _dual("P1")["xh"])  # (the rows do move the filters)
    for e in range(case["B"]):
        st1, ap1, rows1, seeds1 = ds._inputs(case, [e])
        sb1, mb1 = _setup(case, [e])
        mb1.set_hyper([hyper[e]])
        sb1.set_history(theta=True, filter=True)
        ds._sim(case, sb1, mb1, st1, ap1, rows1, seeds1, T)
        assert np.array_equal(_theta_hist(sb1)[:, 0], th[:, e]) and np.array_equal(_x_hist(sb1, mb1)[:, 0], xh[:, e]), e
        sb1.close()
        mb1.close()


# ------------------------------------------------------------------------------------------------ 9. the classes, the driver, the example
def test_the_history_of_the_class_against_forward_and_step():
    B, T, W = 3, 4, 2
    ep, st0, true = ds._warm_loop(B, W)
    ep.svmpc._ensure_batch(ep.mpf.prior)
    ep._filters(ep.svmpc._states(st0))  # (creates the device batches, so that the deep copies below carry them)
    ep.set_history()
    plain = copy.deepcopy(ep)
    plain.set_history(False, False)
    ticks = copy.deepcopy(ep)
    assert ticks.svmpc._history == (True, True) and plain.svmpc._history == (False, False)
    res = ep.simulate(st0, T, plant_params=true)
    ref = plain.simulate(st0, T, plant_params=true)
    for k in res._fields:  # simulate's result is what it is without recording
        assert torch.equal(torch.nan_to_num(getattr(res, k), nan=7.0), torch.nan_to_num(getattr(ref, k), nan=7.0)), k
    hist = ep.history
    assert sorted(hist) == ["dyn_particles", "theta"] and all(isinstance(v, torch.Tensor) for v in hist.values())
    Mp, P = ep._mb.Mp, ep._mb.P
    assert tuple(hist["theta"].shape) == (T, B) + tuple(ep.theta.shape[1:]) and tuple(hist["dyn_particles"].shape) == (T, B, Mp, P)
    x = st0
    for t in range(T):
        a_seq, _ = ticks.forward(x)
        assert torch.equal(hist["theta"][t], ticks.theta), t
        assert torch.equal(hist["dyn_particles"][t], ticks.dyn_particles), t  # (nothing is noted behind a forward(): a plain read)
        x = res.states[t]
        ticks.step(a_seq[:, 0], x)
    assert torch.equal(ep.theta, ticks.theta)
    with pytest.raises(Exception):  # the copy has recorded nothing
        ticks.history["theta"]
    # theta alone
    ep.set_history(theta=True, filter=False)
    ep.simulate(res.states[-1], 2, plant_params=true, resume=res)
    assert sorted(ep.history) == ["theta"] and tuple(ep.history["theta"].shape)[:2] == (2, B)


def test_the_history_of_the_plain_class_against_optimize_and_tick():
    """BatchSVMPC.history: under one torch seed the class's own loop (test_gpu_svmpc_sim.test_class_simulate_against_its_own_loop)"""
    import torch.distributions as dist

    B, T, warm = 3, 4, 2
    pd = dist.Independent(dist.Uniform(torch.tensor([0.8, 0.8]), torch.tensor([1.2, 1.2])), 1)
    true = torch.tensor([[1.2, 0.8], [0.8, 1.1], [1.0, 1.3]])
    st0 = torch.tensor([[3.0, 0.0], [2.5, 0.2], [3.4, -0.1]])
    sim, _ = ps._mirror(B)
    sim.set_history(theta=True)  # (ahead of the first device call: the batch takes the setting when it is built)
    sim.tick(st0, pd)
    loop, plain = copy.deepcopy(sim), copy.deepcopy(sim)
    plain.set_history(False)
    kw = dict(warm_up=warm, plant_params=true)
    torch.manual_seed(40)
    res = sim.simulate(st0, pd, T, **kw)
    torch.manual_seed(40)
    ref = plain.simulate(st0, pd, T, **kw)
    for k in res._fields:
        assert torch.equal(torch.nan_to_num(getattr(res, k), nan=7.0), torch.nan_to_num(getattr(ref, k), nan=7.0)), k
    h = sim.history
    assert sorted(h) == ["theta"] and tuple(h["theta"].shape) == (T, B) + tuple(sim.theta.shape[1:]) and bool(torch.isfinite(h["theta"]).all())
    torch.manual_seed(40)
    x = st0
    for t in range(T):
        if t < warm:
            loop.optimize(x, pd)
        else:
            loop.tick(x, pd)
        assert torch.equal(h["theta"][t], loop.theta), t
        x = res.states[t]
    with pytest.raises(Exception):  # the copies have recorded nothing
        loop.history
    with pytest.raises(Exception):
        plain.history


def _pendulum_driver_args(B=3, steps=5, W=2):
    """the scenario of test_gpu_svmpc_dual_sim.test_run_pendulum_simulations_against_simulate"""
    from dust_amd.controllers import MultiDISCO
    from dust_amd.costs import PendulumQuadCos
    from dust_amd.inference import MPF, GaussianLikelihood, get_gmm
    from dust_amd.kernels import RBFKernel
    from dust_amd.models import PendulumModel

    N, H, S, M = 2, 4, 8, 2
    g = torch.Generator().manual_seed(3)
    cost = PendulumQuadCos()
    space = PendulumModel()
    ctrl = MultiDISCO(space.observation_space, space.action_space, H, N, S, temperature=1.0, a_cov=4.0 * torch.eye(1), inst_cost_fn=cost.inst_cost,
                      term_cost_fn=cost.term_cost, params_sampling=True, params_samples=M, seed=3)
    prior = get_gmm(torch.zeros(N, H, 1), torch.ones(N), 4.0 * torch.eye(1))
    init = 2.0 * torch.randn(N, H, 1, generator=g)
    start = torch.tensor([3.0, 0.0])
    x0 = 1.0 + 0.1 * torch.randn(B, 8, 2, generator=g)
    mpf = MPF(init_particles=x0[0], likelihood=GaussianLikelihood(initial_obs=start, obs_std=0.1, model=PendulumModel(uncertain_params=("length", "mass")),
                                                                log_space=False), optimizer_class=torch.optim.SGD, lr=1e-3, bw=0.1, bw_scale=1.0)
    truths = [dict(length=0.8 + 0.2 * b, mass=1.3 - 0.2 * b) for b in range(B)]
    model_kwargs = dict(g=10.0, uncertain_params=("length", "mass"))
    svk = dict(init_particles=init, prior=prior, kernel=RBFKernel(), n_steps=1, optimizer_class=torch.optim.SGD, lr=1.0, seeds=[3, 4, 5][:B])
    args = (start, init, model_kwargs, truths, ctrl, svk, dict(alpha=1.0, n_samples=S), mpf)
    kw = dict(mpf_steps=2, episodes=B, steps=steps, warm_up=W, seed=9, init_particles=x0)
    return args, kw, dict(S=S, N=N, x0=x0, truths=truths, model_kwargs=model_kwargs, svk=svk, ctrl=ctrl, init=init, mpf=mpf, start=start)


def test_run_pendulum_simulations_history_in_the_reference_convention(monkeypatch):
    from dust_amd.controllers import BatchDualSVMPC
    from dust_amd.inference import BatchSVMPC, ExponentiatedUtility
    from dust_amd.models import PendulumModel
    from dust_amd.utils import simulations

    B, steps, W = 3, 5, 2
    args, kw, s = _pendulum_driver_args(B, steps, W)
    plain = simulations.run_pendulum_simulations(*args, **kw)
    monkeypatch.setattr(simulations, "_PIECE", 3)  # two pieces: 3 + 2 periods
    data = simulations.run_pendulum_simulations(*args, history=True, **kw)
    # history=False: what the function returned before, key by key; history=True changes the two columns alone
    assert list(plain) == list(data)
    for k in plain:
        if k not in ("DynParticles", "PolParticles"):
            assert np.array_equal(plain[k], data[k], equal_nan=True), k
    assert plain["DynParticles"].shape == (B, 8, 2) and plain["PolParticles"].shape == (B, s["N"])
    assert data["DynParticles"].shape == (B, steps, 8, 2) and data["PolParticles"].shape == (B, steps, s["N"])
    assert np.array_equal(plain["DynParticles"], data["DynParticles"][:, -1]) and np.array_equal(plain["PolParticles"], data["PolParticles"][:, -1])
    # the loop of run_pendulum_simulation on a deep copy: forward(), the plant's state, step(), then the rows the reference stores
    sim_ctrl = copy.deepcopy(s["ctrl"])
    sim_ctrl.a_mat = s["init"].clone()
    sim_ctrl.return_rollouts = False
    sv = BatchSVMPC(B, likelihood=ExponentiatedUtility(alpha=1.0, n_samples=s["S"], controller=sim_ctrl, model=PendulumModel(**s["model_kwargs"])), **s["svk"])
    loop = BatchDualSVMPC(sv, s["mpf"], mpf_steps=2, seed=9, init_particles=s["x0"], warm_up=W)
    x = s["start"].repeat(B, 1)
    for t in range(steps):
        a_seq, pw = loop.forward(x)
        if pw is None:  # warming up: the reference stores no row (simulations.py:122)
            assert t < W and np.isnan(data["PolParticles"][:, t]).all(), t
        else:
            assert np.array_equal(data["PolParticles"][:, t], loop.theta[:, :, 0, 0].numpy()), t
        assert np.array_equal(data["Actions"][:, t], a_seq[:, 0, 0].numpy()), t
        x = torch.from_numpy(np.stack((data["Position"][:, t], data["Speed"][:, t]), 1))
        loop.step(a_seq[:, 0], x)
        assert np.array_equal(data["DynParticles"][:, t], copy.deepcopy(loop).dyn_particles.numpy()), t  # the filter with the pair folded in
    assert np.isfinite(data["DynParticles"]).all() and not np.array_equal(data["DynParticles"][:, 0], data["DynParticles"][:, -1])


def test_the_example_runs_tiny():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "pendulum_posterior_example.py"), "--tiny"], capture_output=True, text=True,
                         timeout=300, env=dict(os.environ, PYTHONPATH=ROOT))
    assert out.returncode == 0, out.stderr[-2000:]
    rows = [line for line in out.stdout.splitlines() if line.strip().startswith("period")]
    assert len(rows) == 3 * 3, out.stdout  # three periods shown, three pendulums
    std = [float(line.split("+-")[1].split()[0]) for line in rows]
    assert np.isfinite(std).all() and min(std) > 0
    assert any("warming up" in line for line in rows) and any("first actions" in line for line in rows)
