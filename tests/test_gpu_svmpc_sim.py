"""The closed-loop episode under the reference's rules on the device (csrc/svmpc_episode.hpp svb_sim_body: svmpc_sim_kernel,
svmpc_skid_nav_sim_kernel, svmpc_rows_sim_kernel; dust_svmpc_batch_simulate, `SvmpcBatch.simulate`, `BatchSVMPC.simulate`,
`run_particle_episodes`): warm-up, the accumulated cost, crash and goal in ONE launch.  Every np.array_equal below is bit for bit.

1.  a simulate call against its periods on a clone: optimize (warm-up, zero action) or tick per period, fed the recorded states; the host
    applies the rules with fp32 numpy replicas and deactivates stopped environments - states, actions, weights, n_run, status, every
    getter, one further tick; the forced events of tests/svmpc_sim_cases.py happen where they were proved; rows past n_run are unwritten;
2.  the cost records: loss is the sequential float32 sum of the cost rows (inf exactly for status 2), every cost against the float64
    restatement within the tolerance measured from that restatement alone, and held away from three wrong variants;
3.  rules off: dust_svmpc_batch_episode's bits;
4.  chaining: two calls are one, split inside the warm-up, at its end and after an environment has stopped;
5.  independence from the batch, from inactive neighbours, from neighbours that stop earlier or later or entered stopped;
6.  sweep rows: environment b is a one-environment batch built with row b's values; the prototype's rows are no rows;
7.  one launch per call, every refusal with no launch and the in-out arrays unchanged;
8.  `BatchSVMPC.simulate` against its own optimize / tick loop, with `resume`, with a deep copy between two calls;
9.  `run_particle_episodes` against a host loop over the class, `load` != 0 included;
10. the example's --tiny.
"""
import copy
import ctypes as C
import functools
import importlib.util
import os

import numpy as np
import pytest
import torch

import svmpc_episode_cases as ec
import svmpc_sim_cases as cases
from helpers import elemerr

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GETTERS = ("THETA", "PRIOR_MEANS", "PRIOR_MIX", "A_MAT", "COSTS", "SCORE", "PHI", "LOG_L", "LOG_P", "A_MIX")


def _L():
    from dust_amd import _lib

    return _lib


def _records(b):
    """every getter; LOG_P is None while no forward of the batch has run (an episode that never left its warm-up)"""
    L = _L()
    out = {}
    for n in GETTERS:
        try:
            out[n] = b.get(getattr(L, "SVB_" + n))
        except L.DustError as e:
            assert n == "LOG_P" and e.status == L.ERR_STATE, n
            out[n] = None
    return out


def _same(x, y, fwd=None):
    """the getters of two batches agree bit for bit; fwd [B] bools: the environments that have run a forward() - LOG_P is written by
    forward() alone, so the row of an environment that stopped while warming up is whatever its batch's memory held"""
    for n in GETTERS:
        if x[n] is None or y[n] is None:
            assert x[n] is None and y[n] is None, n
        elif n == "LOG_P" and fwd is not None:
            assert np.array_equal(x[n][fwd], y[n][fwd]), n
        else:
            assert np.array_equal(x[n], y[n]), n


def _inputs(case, T=None):
    """every environment's own start state, particles, true row, seed and dynamics samples (one more period than T: the further tick)"""
    T = case["T"] if T is None else T
    mu, th = ec.particles(case)
    return dict(st=ec.start_states(case), mu=mu, th=th, plant=ec.plant_rows(case), params=ec.tick_params(case, T + 1),
                seeds=[case["seed"] + 13 * b for b in range(case["B"])])


def _batch(case, inp, envs=None, rows=True, **kw):
    """a batch whose slot k holds environment envs[k] of the case (default: all of them, in order), with the case's rows if it has any"""
    from dust_amd import Context

    L = _L()
    envs = list(range(case["B"])) if envs is None else list(envs)
    c = Context(grid=cases.grid_of(case), **ec.context_kwargs(case, **kw))
    b = c.svmpc_batch(len(envs), seeds=[inp["seeds"][e] for e in envs])
    c.close()
    b.set(L.SVB_THETA, inp["th"][envs])
    b.set(L.SVB_PRIOR_MEANS, inp["mu"][envs])
    b.set(L.SVB_A_MAT, inp["th"][envs])
    if case["rows"] and rows:
        assert envs == list(range(case["B"]))
        b.set_hyper(cases.hyper_rows(b.get_hyper(), case["B"]))
    return b


def _sub(inp, envs, t0=0, t1=None):
    """(states, params [t0:t1], plant rows) of these environments"""
    envs = list(envs)
    return (inp["st"][envs], None if inp["params"] is None else np.ascontiguousarray(inp["params"][t0:t1][:, envs]),
            None if inp["plant"] is None else inp["plant"][envs])


def _rules(case, **kw):
    r = case["rules"]
    return dict(dict(warm_up=r["warm_up"], goal=r["goal"], goal_radius=r["radius"], stop_on_crash=r["crash"]), **kw)


def _written(out, B, T, warm):
    """the records of a simulate call hold values in rows t < n_run[b] (p_weights: from the first tick on) and NaN elsewhere"""
    xs, acts, pw, costs, loss, status, n_run, a_seq = out
    for b in range(B):
        n = int(n_run[b])
        for v in (xs, acts, costs):
            assert np.isfinite(v[:n, b]).all() and np.isnan(v[n:, b]).all(), b
        assert np.isfinite(pw[min(warm, n):n, b]).all() and np.isnan(pw[:min(warm, n), b]).all() and np.isnan(pw[n:, b]).all(), b
        assert np.isfinite(a_seq[b]).all() if n > warm else np.isnan(a_seq[b]).all(), b


@functools.lru_cache(maxsize=None)
def _run(cid):
    """the case's simulate call and, on a clone taken before it, its periods - optimize with a zero action while warming up, the tick
    afterwards - fed the recorded states, the host applying the rules to them; then one further tick on both"""
    case = cases.BY_ID[cid]
    T, B, n, grid = case["T"], case["B"], case["n_steps"], cases.grid_of(case)
    warm = case["rules"]["warm_up"]
    inp = _inputs(case)
    b = _batch(case, inp)
    twin = b.clone()
    st, params, plant = _sub(inp, range(B), 0, T)
    out = b.simulate(st, T, n, params, plant, **_rules(case))
    xs, acts, pw = out[:3]
    on, status, n_run = np.ones(B, bool), np.zeros(B, np.int32), np.zeros(B, np.int32)
    x, periods = st.copy(), []
    for t in range(T):
        if not on.any():
            break
        prm = None if params is None else params[t]
        if t < warm:
            twin.optimize(x, n, params=prm, active=on)
            periods.append((t, on.copy(), None, None))
        else:
            a_t, pw_t = twin.tick(x, n, params=prm, active=on)
            periods.append((t, on.copy(), a_t, pw_t))
        x[on] = xs[t][on]
        n_run[on] += 1
        status[on] = cases.apply_rules(case, xs[t][on], grid)
        on &= status == 0
    res = dict(inp=inp, out=out, periods=periods, status=status, n_run=n_run, after=(_records(b), _records(twin)))
    extra = None if inp["params"] is None else inp["params"][T]
    res["further"] = (b.tick(x, n, params=extra), twin.tick(x, n, params=extra), _records(b), _records(twin))
    b.close()
    twin.close()
    return res


# ------------------------------------------------------------------------------------------------ 1. a call is its periods
@pytest.mark.parametrize("cid", cases.IDS)
def test_simulate_equals_its_periods(cid):
    case, r = cases.BY_ID[cid], _run(cid)
    T, B, f, warm = case["T"], case["B"], ec.family(case), case["rules"]["warm_up"]
    xs, acts, pw, costs, loss, status, n_run, a_seq = r["out"]
    assert xs.shape == (T, B, f["ds"]) and acts.shape == (T, B, f["da"]) and pw.shape == (T, B, case["N"]) and costs.shape == (T, B)
    print(cid, "n_run", n_run.tolist(), "status", status.tolist())
    assert np.array_equal(n_run, r["n_run"]) and np.array_equal(status, r["status"])
    _written(r["out"], B, T, warm)
    last = {}
    for t, on, a_t, pw_t in r["periods"]:
        if a_t is None:  # warm-up: the plant got the zero action
            assert not acts[t][on].any(), t
        else:
            assert np.array_equal(a_t[on, 0], acts[t][on]) and np.array_equal(pw_t[on], pw[t][on]), t
            for e in np.nonzero(on)[0]:
                last[e] = a_t[e]
    for e, v in last.items():
        assert np.array_equal(a_seq[e], v), e
    _same(*r["after"], fwd=n_run > warm)
    (a1, p1), (a2, p2), g1, g2 = r["further"]
    assert np.array_equal(a1, a2) and np.array_equal(p1, p2)
    _same(g1, g2)
    for e, (period, st) in cases.EVENTS.get(cid, {}).items():  # the forced events, where tests/test_svmpc_sim_cpu.py proved them
        assert n_run[e] == period + 1 and status[e] == st, (e, n_run[e], status[e])
    if cid in cases.EVENTS:
        free = [e for e in range(B) if e not in cases.EVENTS[cid]]
        assert all(n_run[e] == T and status[e] == 0 for e in free)
    if cid == "pend":
        assert n_run.tolist() == [T] * B and not acts[:warm].any() and acts[warm:].all()


def _raw(b, case, inp, st, T, n_steps, fill=0.0, rules=None, loss=None, status=None, null=(), flags=0):
    """dust_svmpc_batch_simulate through the raw binding on record arrays filled with `fill`; `rules`: fields that replace the case's;
    `null`: which of states / rules / loss / status / n_run / costs go in as NULL -> dict(code, arrays (states, actions, weights, costs,
    a_seq), loss, status, n_run)"""
    L = _L()
    lib, FP, IP = L.load(), L.FP, C.POINTER(C.c_int)
    B, f, r = b.B, ec.family(case), case["rules"]
    ru = L.EpisodeRules()
    ru.t0, ru.warm_up, ru.stop_on_crash, ru.goal_radius = 0, r["warm_up"], int(r["crash"]), 0.0 if r["radius"] is None else r["radius"]
    if r["goal"] is not None:
        ru.goal[:f["ds"]] = list(r["goal"])
    for k, v in (rules or {}).items():
        if k == "goal":
            ru.goal[:len(v)] = list(v)
        else:
            setattr(ru, k, v)
    rows = min(max(T, 1), case["T"])  # (a refused n_periods reads and writes nothing)
    arrays = tuple(np.full(s, fill, np.float32) for s in ((rows, B, f["ds"]), (rows, B, f["da"]), (rows, B, case["N"]), (rows, B), (B, case["H"], f["da"])))
    xs, acts, pw, cs, sq = arrays
    loss = np.zeros(B, np.float32) if loss is None else loss.copy()
    status = np.zeros(B, np.int32) if status is None else status.copy()
    n_run = np.full(B, -1, np.int32)
    sp = np.ascontiguousarray(st, np.float32)
    prm = None if inp["params"] is None else np.ascontiguousarray(inp["params"][:rows], np.float32)
    plt = None if inp["plant"] is None else np.ascontiguousarray(inp["plant"], np.float32)
    P = lambda name, a: None if (a is None or name in null) else a.ctypes.data_as(FP)
    I = lambda name, a: None if name in null else a.ctypes.data_as(IP)
    code = lib.dust_svmpc_batch_simulate(b._h, P("states", sp), T, n_steps, P("params", prm), P("plant", plt), None if "rules" in null else C.byref(ru),
                                         flags, None, P("xs", xs), P("acts", acts), P("pw", pw), P("costs", cs), P("loss", loss),
                                         I("status", status), I("n_run", n_run), P("a_seq", sq))
    return dict(code=code, arrays=arrays, loss=loss, status=status, n_run=n_run)


def test_rows_past_n_run_keep_a_sentinel():
    """through the raw binding: what the call does not write stays what the caller put there"""
    L = _L()
    case, r = cases.BY_ID["part_warm"], _run("part_warm")
    T, B, n = case["T"], case["B"], case["n_steps"]
    b = _batch(case, r["inp"])
    got = _raw(b, case, r["inp"], r["inp"]["st"], T, n, fill=7.5)
    b.close()
    assert got["code"] == L.OK
    for ours, k in zip(got["arrays"], (0, 1, 2, 3, 7)):
        ref = r["out"][k]
        assert np.array_equal(ours, np.where(np.isnan(ref), np.float32(7.5), ref)), k
    assert np.array_equal(got["n_run"], r["out"][6]) and np.array_equal(got["status"], r["out"][5]) and np.array_equal(got["loss"], r["out"][4])
    assert (got["arrays"][0][2:, :2] == 7.5).all() and (got["arrays"][3][2:, :2] == 7.5).all()  # environments 0 and 1 stopped in period 1


# ------------------------------------------------------------------------------------------------ 2. the cost records
@pytest.mark.parametrize("cid", cases.IDS)
def test_costs_and_loss(cid):
    case, r = cases.BY_ID[cid], _run(cid)
    T, B, grid = case["T"], case["B"], cases.grid_of(case)
    xs, _, _, costs, loss, status, n_run, _ = r["out"]
    tol = cases.cost_tolerance(case)
    prev = np.concatenate((r["inp"]["st"][None], xs[:-1]))
    got, ref, var = [], [], {}
    for b in range(B):
        acc = np.float32(0.0)
        for t in range(int(n_run[b])):
            acc = np.float32(acc + costs[t, b])
        if status[b] == 2:
            assert loss[b] == np.inf and np.isposinf(loss[b]), b
        else:
            assert np.float32(loss[b]) == acc and np.isfinite(loss[b]), (b, loss[b], acc)
        n = int(n_run[b])
        got.append(costs[:n, b])
        ref.append(cases.costs64(case, xs[:n, b].astype(np.float64), grid))
        for k, v in cases.cost_variants(case, prev[:n, b].astype(np.float64), xs[:n, b].astype(np.float64), grid).items():
            var.setdefault(k, []).append(v)
    got, ref = np.concatenate(got), np.concatenate(ref)
    err = elemerr(got, ref)
    far = {k: cases.variant_distance(got, np.concatenate(v), tol) for k, v in var.items()}
    print("%-9s cost err %.2e tol %.2e  " % (cid, err, tol) + "  ".join("%s %.0f" % kv for kv in sorted(far.items())))
    assert err < tol, (cid, err, tol)
    assert set(far) == set(cases.COST_POWER[cid])
    for k, least in cases.COST_POWER[cid].items():
        assert far[k] >= least, (cid, k, far[k], least)


# ------------------------------------------------------------------------------------------------ 3. rules off
@pytest.mark.parametrize("cid", ["pend", "part", "skid_nav", "cart", "one", "pend_rows"])
def test_rules_off_is_the_episode(cid):
    case = cases.BY_ID[cid]
    T, B, n = case["T"], case["B"], case["n_steps"]
    inp = _inputs(case)
    b = _batch(case, inp)
    twin = b.clone()
    st, params, plant = _sub(inp, range(B), 0, T)
    xs, acts, pw, costs, loss, status, n_run, a_seq = b.simulate(st, T, n, params, plant)
    want = twin.episode(st, T, n, params, plant)
    got, ref = _records(b), _records(twin)
    b.close()
    twin.close()
    for u, v in zip((xs, acts, pw, a_seq), want):
        assert np.array_equal(u, v)
    _same(got, ref)
    assert n_run.tolist() == [T] * B and not status.any() and np.isfinite(costs).all() and np.isfinite(loss).all()


# ------------------------------------------------------------------------------------------------ 4. chaining
@pytest.mark.parametrize("cid,T1", [("part_warm", 1), ("part_warm", 2), ("part_warm", 3), ("pend", 2), ("skid_nav", 1)])
def test_two_calls_are_one(cid, T1):
    """T1 inside the warm-up (part_warm 1), at its end (2: environments 0 and 1 have just stopped), after it (3); t0, loss and status carried"""
    case, r = cases.BY_ID[cid], _run(cid)
    T, B, n = case["T"], case["B"], case["n_steps"]
    b = _batch(case, r["inp"])
    st, p1, plant = _sub(r["inp"], range(B), 0, T1)
    _, p2, _ = _sub(r["inp"], range(B), T1, T)
    one = b.simulate(st, T1, n, p1, plant, **_rules(case))
    x = st.copy()
    for e in range(B):
        if one[6][e] > 0:
            x[e] = one[0][one[6][e] - 1, e]
    two = b.simulate(x, T - T1, n, p2, plant, **_rules(case, t0=T1, loss=one[4], status=one[5]))
    got = _records(b)
    b.close()
    whole = r["out"]
    for k in range(4):  # states, actions, weights, costs: the rows of both calls, NaN where neither wrote
        assert np.array_equal(np.concatenate((one[k], two[k])), whole[k], equal_nan=True), k
    assert np.array_equal(two[4], whole[4]) and np.array_equal(two[5], whole[5])
    assert np.array_equal(one[6] + two[6], whole[6])
    for e in range(B):  # a_seq: of the call that ran the environment's last forward()
        src = two[7][e] if not np.isnan(two[7][e]).any() else one[7][e]
        assert np.array_equal(src, whole[7][e], equal_nan=True), e
    _same(got, r["after"][0], fwd=whole[6] > case["rules"]["warm_up"])


# ------------------------------------------------------------------------------------------------ 5. independence from the batch
@pytest.mark.parametrize("cid", ["part_warm", "pend", "skid_nav"])
def test_an_environment_does_not_depend_on_its_batch(cid):
    case, r = cases.BY_ID[cid], _run(cid)
    # e: an environment that runs into the ticks (its LOG_P is then defined), other: a neighbour that stops at another time - part_warm:
    # environment 0 stops in period 1, environment 2 runs to T; skid_nav: environment 1 crashes in period 0
    e, other = {"part_warm": (2, 0), "pend": (1, 0), "skid_nav": (0, 1)}[cid]
    T, n, inp = case["T"], case["n_steps"], r["inp"]
    assert r["out"][6][e] > case["rules"]["warm_up"]

    def sim(b, envs, **kw):
        st, params, plant = _sub(inp, envs, 0, T)
        return b.simulate(st, T, n, params, plant, **_rules(case, **kw))

    ref = {k: v[e] for k, v in r["after"][0].items()}

    def check(out, got, slot, env=e, records=ref):
        for k in range(4):
            assert np.array_equal(out[k][:, slot], r["out"][k][:, env], equal_nan=True), (k, slot)
        for k in (4, 5, 6, 7):
            assert np.array_equal(out[k][slot], r["out"][k][env], equal_nan=True), (k, slot)
        if records is not None:
            for k in GETTERS:
                assert (got[k] is None and records[k] is None) or np.array_equal(got[k][slot], records[k]), (k, slot)

    alone = _batch(case, inp, [e])
    check(sim(alone, [e]), _records(alone), 0)
    alone.close()
    envs = [e, other, e, (e + 1) % case["B"], e]  # slots 0 / 2 / 4 of five
    five = _batch(case, inp, envs)
    out, got = sim(five, envs), _records(five)
    five.close()
    for slot in (0, 2, 4):
        check(out, got, slot)
    check(out, got, 1, env=other, records=None)  # ... and the neighbour that stops at another time is itself
    # beside an inactive neighbour and one that entered stopped: a tick first, so that they have getters to keep
    envs = [other, e, other]
    three = _batch(case, inp, envs)
    st, params, _ = _sub(inp, envs, 0, 1)
    lone = _batch(case, inp, [e])
    three.tick(st, n, params=None if params is None else params[0])
    lone.tick(st[1:2], n, params=None if params is None else params[0][1:2])
    before = _records(three)
    entered = dict(loss=np.array([0.0, 0.0, 3.25], np.float32), status=np.array([0, 0, 1], np.int32))
    out, got = sim(three, envs, active=[0, 1, 1], **entered), _records(three)
    solo, solo_got = sim(lone, [e]), _records(lone)
    three.close()
    lone.close()
    for k in range(4):
        assert np.array_equal(out[k][:, 1], solo[k][:, 0], equal_nan=True) and np.isnan(out[k][:, [0, 2]]).all(), k
    for k in (4, 5, 6, 7):
        assert np.array_equal(out[k][1], solo[k][0], equal_nan=True), k
    assert np.isnan(out[7][[0, 2]]).all() and out[6].tolist()[0] == -1 and out[6].tolist()[2] == 0  # (inactive: unwritten; stopped: no period)
    assert out[4][2] == np.float32(3.25) and out[5][2] == 1 and out[4][0] == 0 and out[5][0] == 0
    for k in GETTERS:
        assert np.array_equal(got[k][1], solo_got[k][0]), k
        assert np.array_equal(got[k][[0, 2]], before[k][[0, 2]]), k


# ------------------------------------------------------------------------------------------------ 6. sweep rows
def test_sweep_rows():
    case, r = cases.BY_ID["pend_rows"], _run("pend_rows")
    T, B, n, inp = case["T"], case["B"], case["n_steps"], r["inp"]
    probe = _batch(case, inp)
    rows = probe.get_hyper()
    probe.close()
    changed = 0
    for e in range(B):  # environment e against a one-environment batch whose PROTOTYPE carries row e's values: the uniform instance
        lone = _batch(case, inp, [e], rows=False, **cases.row_kwargs(rows, e))
        st, params, plant = _sub(inp, [e], 0, T)
        out = lone.simulate(st, T, n, params, plant, **_rules(case))
        got = _records(lone)
        lone.close()
        for k in range(4):
            assert np.array_equal(out[k][:, 0], r["out"][k][:, e], equal_nan=True), (k, e)
        for k in (4, 5, 6, 7):
            assert np.array_equal(out[k][0], r["out"][k][e], equal_nan=True), (k, e)
        for k in GETTERS:
            assert np.array_equal(got[k][0], r["after"][0][k][e]), (k, e)
    # rows equal to the prototype's: the batch without rows (the uniform instances), bit for bit - and the case's rows do change the result
    plain, same = _batch(case, inp, rows=False), _batch(case, inp, rows=False)
    same.set_hyper(same.get_hyper())
    st, params, plant = _sub(inp, range(B), 0, T)
    u, v = plain.simulate(st, T, n, params, plant, **_rules(case)), same.simulate(st, T, n, params, plant, **_rules(case))
    gu, gv = _records(plain), _records(same)
    plain.close()
    same.close()
    for k in range(8):
        assert np.array_equal(u[k], v[k], equal_nan=True), k
    _same(gu, gv)
    assert np.array_equal(u[1][:, 0], r["out"][1][:, 0])  # row 0 holds the prototype's values
    for e in range(1, B):
        changed += not np.array_equal(u[1][:, e], r["out"][1][:, e])
    assert changed == B - 1


# ------------------------------------------------------------------------------------------------ 7. launches and refusals
def test_one_launch_per_call_and_refusals_before_any_launch():
    L = _L()
    case = cases.BY_ID["part_warm"]
    inp = _inputs(case)
    B, n, T = case["B"], case["n_steps"], case["T"]
    b = _batch(case, inp)
    b.ctx.profile(True)
    count = lambda: b.ctx.profile_get().get("svmpc_batch_kernel", (0.0, 0))[1]
    total = lambda: sum(v[1] for v in b.ctx.profile_get().values())
    st, params, plant = _sub(inp, range(B), 0, T)
    b.simulate(st, 1, n, None, None, **_rules(case))
    assert count() == 1 == total()
    b.simulate(st, T, n, None, None, **_rules(case))
    assert count() == 2 == total()
    before = _records(b)
    nan = float("nan")
    refusals = [
        (dict(null=("states",)), L.ERR_INVALID), (dict(null=("xs",)), L.ERR_INVALID), (dict(null=("acts",)), L.ERR_INVALID),
        (dict(n_steps=0), L.ERR_INVALID), (dict(T=0), L.ERR_INVALID), (dict(T=4097), L.ERR_INVALID),
        (dict(flags=L.SVMPC_BATCH_KEEP_ACTIONS), L.ERR_UNSUPPORTED), (dict(flags=L.PTR_DEVICE), L.ERR_UNSUPPORTED),
        (dict(null=("rules",)), L.ERR_INVALID), (dict(null=("loss",)), L.ERR_INVALID), (dict(null=("status",)), L.ERR_INVALID),
        (dict(null=("n_run",)), L.ERR_INVALID), (dict(null=("costs",)), L.ERR_INVALID),
        (dict(rules=dict(t0=-1)), L.ERR_INVALID), (dict(rules=dict(warm_up=-1)), L.ERR_INVALID),
        (dict(rules=dict(goal_radius=nan)), L.ERR_INVALID), (dict(rules=dict(goal_radius=float("inf"))), L.ERR_INVALID),
        (dict(rules=dict(goal=(9.0, nan, 0.0, 0.0))), L.ERR_INVALID),
        (dict(status=np.array([0, 3, 0], np.int32)), L.ERR_INVALID), (dict(status=np.array([-1, 0, 0], np.int32)), L.ERR_INVALID),
    ]
    loss_in = np.array([1.5, 2.5, 3.5], np.float32)
    for kw, want in refusals:
        kw = dict(dict(status=np.array([0, 1, 2], np.int32)), **kw)
        got = _raw(b, case, inp, st, kw.pop("T", T), kw.pop("n_steps", n), fill=7.5, loss=loss_in, **kw)
        assert got["code"] == want, (kw, got["code"], want)
        assert np.array_equal(got["loss"], loss_in) and np.array_equal(got["status"], kw["status"]) and (got["n_run"] == -1).all(), kw
        assert all((a == 7.5).all() for a in got["arrays"]), kw  # nothing was written
    assert count() == 2 == total()
    _same(_records(b), before)
    b.close()
    # the crash rule needs a map: a Pendulum batch has none
    pend = cases.BY_ID["pend"]
    ip = _inputs(pend)
    bp = _batch(pend, ip)
    bp.ctx.profile(True)
    sp, pp, lp = _sub(ip, range(pend["B"]), 0, pend["T"])
    with pytest.raises(L.DustError) as e:
        bp.simulate(sp, pend["T"], pend["n_steps"], pp, lp, stop_on_crash=True)
    assert e.value.status == L.ERR_UNSUPPORTED
    with pytest.raises(L.DustError) as e:  # what the episode entry refuses: uncertain parameters without rows
        bp.simulate(sp, pend["T"], pend["n_steps"], None, lp)
    assert e.value.status == L.ERR_INVALID
    assert sum(v[1] for v in bp.ctx.profile_get().values()) == 0
    bp.close()


# ------------------------------------------------------------------------------------------------ 8. the class
def _mirror(n_envs, seed=0, N=3, S=16, H=6, M=3):
    from dust_amd.controllers import MultiDISCO
    from dust_amd.costs import PendulumQuadCos
    from dust_amd.inference import BatchSVMPC, ExponentiatedUtility, get_gmm
    from dust_amd.kernels import RBFKernel
    from dust_amd.models import PendulumModel

    model, cost = PendulumModel(uncertain_params=("length", "mass")), PendulumQuadCos()
    ctrl = MultiDISCO(model.observation_space, model.action_space, H, N, S, temperature=1.0, a_cov=4.0 * torch.eye(1), inst_cost_fn=cost.inst_cost,
                      term_cost_fn=cost.term_cost, params_sampling=True, params_samples=M, seed=seed)
    g = torch.Generator().manual_seed(3)
    mu = torch.randn(N, H, 1, generator=g)
    th = mu + 2 * torch.randn(N, H, 1, generator=g)
    ctrl.a_mat = th.clone()
    prior = get_gmm(mu, torch.ones(N), 4.0 * torch.eye(1))
    lik = ExponentiatedUtility(alpha=1.0, n_samples=S, controller=ctrl, model=model)
    return BatchSVMPC(n_envs, init_particles=th, prior=prior, likelihood=lik, kernel=RBFKernel(), n_particles=N, n_steps=2,
                      optimizer_class=torch.optim.Adam, lr=0.1), cost


def _eq(u, v):
    return torch.equal(torch.nan_to_num(u.float(), nan=7.0, posinf=8.0), torch.nan_to_num(v.float(), nan=7.0, posinf=8.0))


def test_class_simulate_against_its_own_loop():
    """simulate(T) draws its dynamics samples as T calls of optimize() / tick() do: under one torch seed the class's own loop, fed the
    recorded states, gives the same actions, weights and costs; resume: twice against once; a deep copy between two calls"""
    import torch.distributions as dist

    B, T, warm = 3, 4, 2
    pd = dist.Independent(dist.Uniform(torch.tensor([0.8, 0.8]), torch.tensor([1.2, 1.2])), 1)
    true = torch.tensor([[1.2, 0.8], [0.8, 1.1], [1.0, 1.3]])
    st0 = torch.tensor([[3.0, 0.0], [2.5, 0.2], [3.4, -0.1]])
    sim, cost = _mirror(B)
    sim.tick(st0, pd)  # (creates the device batch, so that the deep copies below carry one)
    loop, halves = copy.deepcopy(sim), copy.deepcopy(sim)
    kw = dict(warm_up=warm, goal=torch.zeros(2), goal_radius=0.5, plant_params=true)
    torch.manual_seed(40)
    res = sim.simulate(st0, pd, T, **kw)
    after = torch.rand(1)
    assert res.t0 == T and tuple(res.states.shape) == (T, B, 2) and tuple(res.costs.shape) == (T, B) and res.n_run.tolist() == [T] * B
    torch.manual_seed(40)
    x, acc = st0, torch.zeros(B)
    for t in range(T):
        if t < warm:
            loop.optimize(x, pd)
            assert not bool(res.actions[t].any()) and bool(torch.isnan(res.p_weights[t]).all())
        else:
            a_t, pw_t = loop.tick(x, pd)
            assert torch.equal(a_t[:, 0], res.actions[t]) and torch.equal(pw_t, res.p_weights[t]), t
        x = res.states[t]
        c = cost.inst_cost(x)  # the controller's own cost function on the recorded state, on the host
        assert float((c.reshape(B) - res.costs[t]).abs().max()) <= 1e-4 * float(c.abs().max())
        acc = acc + res.costs[t]
    assert torch.equal(acc, res.loss) and torch.equal(a_t, res.a_seq) and torch.equal(torch.rand(1), after)
    assert torch.equal(sim.theta, loop.theta)
    # resume: 1 + 3 periods against the 4, the second half on a deep copy taken between the two calls
    torch.manual_seed(40)
    h1 = halves.simulate(st0, pd, 1, **kw)
    twin = copy.deepcopy(halves)
    state = torch.get_rng_state()
    h2 = halves.simulate(h1.states[-1], pd, T - 1, resume=h1, **kw)
    torch.set_rng_state(state)
    h2t = twin.simulate(h1.states[-1], pd, T - 1, resume=h1, **kw)
    assert h2.t0 == T and all(_eq(u, v) for u, v in zip(h2, h2t)) and torch.equal(halves.theta, twin.theta)
    for k in range(4):
        assert _eq(torch.cat((h1[k], h2[k])), res[k]), k
    assert torch.equal(h2.loss, res.loss) and torch.equal(h2.status, res.status) and torch.equal(h2.a_seq, res.a_seq)
    assert torch.equal(halves.theta, sim.theta)


# ------------------------------------------------------------------------------------------------ 9. run_particle_episodes
def _particle_batch(B, N=3, S=16, H=5, M=2):
    import torch.distributions as dist

    import amppi_cases as ac
    from dust_amd.controllers import MultiDISCO
    from dust_amd.inference import BatchSVMPC, ExponentiatedUtility, get_gmm
    from dust_amd.kernels import RBFKernel
    from dust_amd.models import Particle

    model = Particle(**ac.PART_ENV, mass=2.0, uncertain_params=("mass",))
    ctrl = MultiDISCO(model.observation_space, model.action_space, H, N, S, temperature=1.0, a_cov=25.0 * torch.eye(2), inst_cost_fn=model.default_inst_cost,
                      term_cost_fn=model.default_term_cost, params_sampling=True, params_samples=M, seed=5)
    g = torch.Generator().manual_seed(9)
    th = 3.0 * torch.randn(N, H, 2, generator=g)
    ctrl.a_mat = th.clone()
    prior = get_gmm(th.clone(), torch.ones(N), 25.0 * torch.eye(2))
    lik = ExponentiatedUtility(alpha=1.0, n_samples=S, controller=ctrl, model=model)
    pd = dist.Independent(dist.Uniform(torch.tensor([1.5]), torch.tensor([2.5])), 1)
    return BatchSVMPC(B, init_particles=th, prior=prior, likelihood=lik, kernel=RBFKernel(), n_particles=N, n_steps=1,
                      optimizer_class=torch.optim.SGD, lr=1.0), model, pd


def test_run_particle_episodes_against_a_host_loop():
    """the batched twin of run_particle_episode against the reference's loop written over the class - optimize, forward once warmed up,
    cost, crash, goal -, with Particle.step replaced by the recorded states (the plant is checked in test 2 and in
    test_gpu_svmpc_episode.py).  load != 0 shows as the second piece's plant rows: the recorded states of both pieces are reproduced
    by the float64 step under mass and mass + load, and not under the mass alone."""
    from dust_amd.utils import simulations as sims

    case = cases.BY_ID["part_warm"]
    st0 = torch.tensor(case["start"])
    B, steps, warm, load = 3, 8, 2, 1.5
    bs, model, pd = _particle_batch(B)
    bs.tick(st0, pd)
    loop = copy.deepcopy(bs)
    seen = []
    real = bs.simulate
    bs.simulate = lambda *a, **k: seen.append(real(*a, **k)) or seen[-1]
    torch.manual_seed(50)
    losses = sims.run_particle_episodes(st0, model, pd, bs, warm_up=warm, load=load, steps=steps)
    assert [int(r.states.shape[0]) for r in seen] == [steps // 4, steps - steps // 4] and seen[-1].t0 == steps
    xs = torch.cat([r.states for r in seen])
    acts = torch.cat([r.actions for r in seen])
    n_run = sum(r.n_run for r in seen)
    # the reference's loop over the class, environment by environment through `active`
    torch.manual_seed(50)
    cum, on, x = torch.zeros(B), np.ones(B, bool), st0.clone()
    for step in range(steps):
        if step < warm:
            loop.optimize(x, pd)  # (simulate draws for every environment of its mask, stopped or not: so does this loop)
            a = torch.zeros(B, 2)
        else:
            a_seq, _ = loop.tick(x, pd)
            a = a_seq[:, 0]
        for b in np.nonzero(on)[0]:
            assert torch.equal(a[b], acts[step, b]), (step, b)
            x[b] = xs[step, b]
            cum[b] = cum[b] + model.default_inst_cost(x[b].view(1, -1)).reshape(())
            if bool(model.obst_map.get_collisions(x[b, :2])):
                cum[b], on[b] = float("inf"), False
            elif float((model.target - x[b]).norm()) <= 1.0:
                on[b] = False
            if not on[b]:
                assert n_run[b] == step + 1, (b, step)
    print("losses", losses.tolist(), "host", cum.tolist(), "n_run", n_run.tolist())
    assert losses[0] == float("inf") and cum[0] == float("inf") and n_run.tolist() == [2, 2, steps]
    # (every device cost lies within the cost tolerance, at most TOL_CAP, of the host's; the terms are not negative: so does their sum)
    assert torch.allclose(losses[1:], cum[1:], rtol=ec.TOL_CAP, atol=0)
    # the load: environment 2's states of the second piece follow mass + load
    grid = cases.grid_of(case)
    prev = torch.cat((st0[None], xs[:-1]))[:, 2].numpy().astype(np.float64)
    a2 = acts[:, 2].numpy().astype(np.float64)
    tol = ec.TOL_CAP
    for t in range(steps):
        heavy = t >= steps // 4
        step = lambda m: ec.plant_step(dict(case, up=("mass",)), prev[t:t + 1], a2[t:t + 1], np.array([[m]]), grid)
        assert elemerr(xs[t, 2:3].numpy(), step(2.0 + load if heavy else 2.0)) < tol, t
    # (the tick periods of the second piece: the action is not zero, so the mass shows - in at least one of them by 5 tolerances)
    light = [elemerr(xs[t, 2:3].numpy(), ec.plant_step(dict(case, up=("mass",)), prev[t:t + 1], a2[t:t + 1], np.array([[2.0]]), grid)) for t in range(warm, steps)]
    print("distance from the unloaded plant, in tolerances:", [round(v / tol, 1) for v in light])
    assert max(light) > 5 * tol


# ------------------------------------------------------------------------------------------------ 10. the example
def test_example_runs_tiny():
    path = os.path.join(ROOT, "examples", "particle_sweep_example.py")
    spec = importlib.util.spec_from_file_location("particle_sweep_example", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    losses, table = mod.run(quiet=True, **mod.TINY)
    B = mod.TINY["n_trials"]
    assert tuple(losses.shape) == (B,) and len(table) == B and not bool(torch.isnan(losses).any())
    assert [row["loss"] for row in table] == sorted(row["loss"] for row in table)
