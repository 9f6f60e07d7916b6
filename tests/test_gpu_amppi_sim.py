"""AMPPI episodes under the reference's rules on the device (csrc/amppi_episode.hpp amppi_sim_period_kernel /
amppi_skid_nav_sim_period_kernel, dust_amppi_batch_simulate, `AmppiBatch.simulate`, `BatchAMPPI.simulate`, `run_particle_episodes`): T
periods of tick, plant step, cost, crash and goal, one launch per period and no host between two periods.  Every np.array_equal below is
bit for bit; the cases and why each exists are in tests/amppi_sim_cases.py.

1. a call is its periods: simulate(T) against (update of a clone fed the call's own recorded states, then roll) per period, with the
   rules applied on the host through the fp32 replicas and stopped environments deactivated - costs, omega, actions, sequences,
   get_actions, n_run, status, one further tick on both; rows past n_run stay the sentinel;
2. loss and cost: the loss is the sequential fp32 sum of the recorded costs (inf after a crash); every cost against the float64
   restatement on the device's own state, held away from three wrong costs; every state within the plant tolerance;
3. rules off: the call is dust_amppi_batch_episode; 4. two chained calls are one; 5. an environment does not depend on its batch;
6. T launches per call whatever stops, every refusal before any launch; 7. the class, the driver, the example.
"""
import copy
import functools
import importlib.util
import os

import numpy as np
import pytest
import torch

import amppi_cases as ac
import amppi_sim_cases as cases
from helpers import elemerr

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("xs", "acts", "costs", "omega", "ic", "loss", "status", "n_run", "a_seq")


def _L():
    from dust_amd import _lib

    return _lib


def _inputs(case):
    """every environment's own start state, sequence, true row, seed and parameter rows (one more period than T: the further tick)"""
    return dict(st=cases.start_states(case), a0=cases.start_sequences(case), plant=cases.plant_rows(case),
                params=cases.tick_params(case, case["T"] + 1), seeds=[case["seed"] + 13 * b for b in range(case["B"])])


def _batch(case, inp, envs=None):
    """a batch whose slot k holds environment envs[k] of the case (default: all of them, in order)"""
    from dust_amd import Context

    envs = list(range(case["B"])) if envs is None else list(envs)
    c = Context(grid=cases.grid_of(case), **cases.context_kwargs(case))
    if case["mode"] == "ut":
        c.set_param_weights(np.asarray(ac.weights(len(case["up"]))[0], np.float32))
    b = c.amppi_batch(len(envs), [inp["seeds"][e] for e in envs])
    c.close()
    b.set_a_seq(inp["a0"][envs])
    return b


def _sub(inp, envs, t0=0, t1=None):
    envs = list(envs)
    return (inp["st"][envs], None if inp["params"] is None else np.ascontiguousarray(inp["params"][t0:t1][:, envs]),
            None if inp["plant"] is None else inp["plant"][envs])


def _kw(case, rules=True):
    r = case["rules"]
    kw = dict(shared_params=case["mode"] == "single", roll_steps=case["roll_steps"])
    if rules:
        kw.update(goal=r["goal"], goal_radius=r["radius"], stop_on_crash=r["crash"])
    return kw


def _sim(b, case, inp, envs, t0=0, t1=None, states=None, plant=None, rules=True, **extra):
    t1 = case["T"] if t1 is None else t1
    st, params, pl = _sub(inp, envs, t0, t1)
    out = b.simulate(st if states is None else states, t1 - t0, params, plant_params=pl if plant is None else plant, t0=t0, **_kw(case, rules), **extra)
    return dict(zip(NAMES, out))


def _carry(prev, x):
    """the states a chained call starts from: where every environment stands"""
    x = np.array(x, np.float32)
    for e in range(x.shape[0]):
        if prev["n_run"][e] > 0:
            x[e] = prev["xs"][prev["n_run"][e] - 1, e]
    return x


@functools.lru_cache(maxsize=None)
def _run(cid):
    """the case's call and, on a clone taken before it, its periods: update fed the recorded states, roll, the rules on the host"""
    case = cases.BY_ID[cid]
    T, B, roll, grid = case["T"], case["B"], case["roll_steps"], cases.grid_of(case)
    inp = _inputs(case)
    b = _batch(case, inp)
    twin = b.clone()
    st, params, _ = _sub(inp, range(B), 0, T)
    r = _sim(b, case, inp, range(B))
    on, x = np.ones(B, bool), st.copy()
    host = dict(status=np.zeros(B, np.int32), n_run=np.zeros(B, np.int32), ticks=[], last_acts=[None] * B, last_seq=[None] * B)
    for t in range(T):
        if not on.any():
            break
        c_t, o_t, s_t, _ = twin.update(x, None, None if params is None else params[t], shared_params=case["mode"] == "single", active=on.astype(np.uint8))
        drawn = twin.get_actions()
        twin.roll(roll, active=on.astype(np.uint8))
        host["ticks"].append((on.copy(), c_t, o_t, s_t))
        for e in np.nonzero(on)[0]:
            host["last_acts"][e], host["last_seq"][e] = drawn[e], s_t[e]
            assert np.isfinite(r["xs"][t, e]).all(), (t, e)
            x[e] = r["xs"][t, e]
        stat = cases.apply_rules(case, x, grid)
        host["n_run"][on] += 1
        stop = on & (stat != 0)
        host["status"][stop] = stat[stop]
        on &= ~stop
    out = dict(r, inp=inp, host=host, x_end=x, after=((b.get_a_seq(), b.get_actions()), twin.get_a_seq()))
    extra = None if inp["params"] is None else inp["params"][T]
    kw = dict(shared_params=case["mode"] == "single", want_actions=True)
    out["further"] = (b.update(x, None, extra, **kw), twin.update(x, None, extra, **kw))
    b.close()
    twin.close()
    return out


# ------------------------------------------------------------------------------------------------ 1. a call is its periods
@pytest.mark.parametrize("cid", cases.IDS)
def test_call_equals_its_periods(cid):
    case, r = cases.BY_ID[cid], _run(cid)
    T, B, h = case["T"], case["B"], _run(cid)["host"]
    assert np.array_equal(r["n_run"], h["n_run"]) and np.array_equal(r["status"], h["status"]), (r["n_run"], h["n_run"], r["status"], h["status"])
    for t, (on, c_t, o_t, s_t) in enumerate(h["ticks"]):
        for e in np.nonzero(on)[0]:
            assert np.array_equal(c_t[e], r["costs"][t, e]) and np.array_equal(o_t[e], r["omega"][t, e]), (t, e)
            assert np.array_equal(s_t[e, 0], r["acts"][t, e]), (t, e)
    for e in range(B):
        n = r["n_run"][e]
        assert n >= 1
        for k in ("xs", "acts", "costs", "omega", "ic"):  # rows past n_run are still the sentinel, the rows before it are written
            assert np.isnan(r[k][n:, e]).all() and np.isfinite(r[k][:n, e]).all(), (k, e)
        assert np.array_equal(r["a_seq"][e], h["last_seq"][e]), e
        assert np.array_equal(r["after"][0][1][e], h["last_acts"][e]), e  # get_actions: the environment's last period
    assert np.array_equal(r["after"][0][0], r["after"][1])  # the sequences after the rolls
    for u, v in zip(*r["further"]):
        assert np.array_equal(u, v)
    want = cases.EVENTS.get(cid)
    if want is not None:
        for e in range(B):
            period, status = want.get(e, (T - 1, 0))
            assert (r["n_run"][e], r["status"][e]) == (period + 1, status), (e, r["n_run"][e], r["status"][e])
    elif not case["rules"]["crash"] and case["rules"]["goal"] is None:
        assert (r["n_run"] == T).all() and not r["status"].any()


# ------------------------------------------------------------------------------------------------ 2. loss and cost
@pytest.mark.parametrize("cid", cases.IDS)
def test_loss_and_cost(cid):
    case, r = cases.BY_ID[cid], _run(cid)
    grid, tol = cases.grid_of(case), cases.cost_tolerance(case)
    new, prev, got, ref_x = [], [], [], []
    x0, rows = r["inp"]["st"], r["inp"]["plant"]
    pgrid = grid if case["family"] == "particle" else None
    for e in range(case["B"]):
        n = int(r["n_run"][e])
        want = np.float32(np.inf) if r["status"][e] == 2 else cases.loss32(r["ic"][:, e], n)
        assert np.array_equal(r["loss"][e], want), (e, r["loss"][e], want)
        for t in range(n):
            p = x0[e] if t == 0 else r["xs"][t - 1, e]
            prev.append(p)
            new.append(r["xs"][t, e])
            got.append(r["ic"][t, e])
            ref_x.append(cases.plant_step(case, p[None], r["acts"][t, e][None], None if rows is None else rows[e:e + 1], pgrid)[0])
    new, prev, got = np.array(new, np.float64), np.array(prev, np.float64), np.array(got)
    ref = cases.costs64(case, new, grid)
    err, perr, ptol = elemerr(got, ref), elemerr(new, np.array(ref_x)), cases.plant_tolerance(case)
    far = {k: cases.variant_distance(ref, v, tol) for k, v in cases.cost_variants(case, prev, new, grid).items()}
    print("%-9s cost err %.2e tol %.2e plant err %.2e tol %.2e  " % (cid, err, tol, perr, ptol) + "  ".join("%s %.0f" % kv for kv in sorted(far.items())))
    assert err < tol, (cid, err, tol)
    assert perr < ptol, (cid, perr, ptol)
    for k, v in far.items():
        if cases.shows(case, k):
            assert v >= cases.COST_POWER, (cid, k, v)
            assert cases.variant_distance(got, cases.cost_variants(case, prev, new, grid)[k], tol) >= cases.COST_POWER, (cid, k)


# ------------------------------------------------------------------------------------------------ 3. rules off
@pytest.mark.parametrize("cid", ["pend257", "part_map", "skid_nav", "pend_ut", "roll3"])
def test_rules_off_is_the_plain_episode(cid):
    case = cases.BY_ID[cid]
    inp, envs = _inputs(case), range(case["B"])
    a, b = _batch(case, inp), _batch(case, inp)
    r = _sim(a, case, inp, envs, rules=False)
    st, params, plant = _sub(inp, envs, 0, case["T"])
    xs, acts, costs, omega, a_seq = b.episode(st, case["T"], params, plant_params=plant, roll_steps=case["roll_steps"], shared_params=case["mode"] == "single")
    for u, v in ((r["xs"], xs), (r["acts"], acts), (r["costs"], costs), (r["omega"], omega), (r["a_seq"], a_seq), (a.get_a_seq(), b.get_a_seq()),
                 (a.get_actions(), b.get_actions())):
        assert np.array_equal(u, v)
    assert (r["n_run"] == case["T"]).all() and not r["status"].any() and np.isfinite(r["loss"]).all()
    a.close()
    b.close()


# ------------------------------------------------------------------------------------------------ 4. chained calls
@pytest.mark.parametrize("cid,cut", [("part_map", 1), ("part_map", 2), ("cart1021", 1), ("roll3", 2)])
def test_two_chained_calls_are_one(cid, cut):
    """split before and behind a stop (part_map: environments 0 and 1 stop in period 0, environment 2 in period 1)"""
    case, r = cases.BY_ID[cid], _run(cid)
    inp, envs, T = r["inp"], range(case["B"]), case["T"]
    b = _batch(case, inp)
    one = _sim(b, case, inp, envs, 0, cut)
    two = _sim(b, case, inp, envs, cut, T, states=_carry(one, inp["st"]), loss=one["loss"], status=one["status"])
    for e in envs:
        n1, n2 = int(one["n_run"][e]), int(two["n_run"][e])
        assert n1 + n2 == r["n_run"][e] and (n2 == 0 or n1 == cut), e
        for k in ("xs", "acts", "costs", "omega", "ic"):
            assert np.array_equal(np.concatenate((one[k][:n1, e], two[k][:n2, e])), r[k][:n1 + n2, e]), (k, e)
        assert np.array_equal((two if n2 else one)["a_seq"][e], r["a_seq"][e]), e
        if n2 == 0:  # an environment that enters stopped writes n_run = 0 and nothing else
            assert np.isnan(two["a_seq"][e]).all() and np.isnan(two["xs"][:, e]).all()
    assert np.array_equal(two["loss"], r["loss"]) and np.array_equal(two["status"], r["status"])
    assert np.array_equal(b.get_a_seq(), r["after"][0][0])
    b.close()


def test_a_changed_plant_is_two_chained_calls():
    """Particle with other true rows from period 1 on: split once or twice, the same"""
    case = cases.BY_ID["part_map"]
    inp, envs, T = _inputs(case), range(case["B"]), case["T"]
    heavy = (inp["plant"] + np.float32(0.5)).astype(np.float32)
    a, b = _batch(case, inp), _batch(case, inp)
    a1 = _sim(a, case, inp, envs, 0, 1)
    a2 = _sim(a, case, inp, envs, 1, T, states=_carry(a1, inp["st"]), plant=heavy, loss=a1["loss"], status=a1["status"])
    b1 = _sim(b, case, inp, envs, 0, 1)
    b2 = _sim(b, case, inp, envs, 1, 2, states=_carry(b1, inp["st"]), plant=heavy, loss=b1["loss"], status=b1["status"])
    b3 = _sim(b, case, inp, envs, 2, T, states=_carry(b2, _carry(b1, inp["st"])), plant=heavy, loss=b2["loss"], status=b2["status"])
    assert np.array_equal(a2["loss"], b3["loss"]) and np.array_equal(a2["status"], b3["status"])
    assert np.array_equal(a2["n_run"], b2["n_run"] + b3["n_run"]) and np.array_equal(a.get_a_seq(), b.get_a_seq())
    e = 3  # the environment that runs on: its states under the heavier plant differ from the one-plant call's
    assert np.array_equal(a2["xs"][:, e], np.concatenate((b2["xs"][:1, e], b3["xs"][:1, e])))
    assert not np.array_equal(a2["xs"][:, e], _run("part_map")["xs"][1:, e])
    a.close()
    b.close()


# ------------------------------------------------------------------------------------------------ 5. independence from the batch
def test_an_environment_does_not_depend_on_its_batch():
    """environment 2 of part_map (a crash in period 1): alone, in slots 0 / 2 / 4 of five beside an earlier-stopping and a never-stopping
    neighbour, beside inactive and already-stopped neighbours, and from a clone taken between two calls"""
    case, r = cases.BY_ID["part_map"], _run("part_map")
    inp, e, T = r["inp"], 2, case["T"]
    want = {k: r[k][:, e] for k in ("xs", "acts", "costs", "omega", "ic")}
    want.update({k: r[k][e] for k in ("loss", "status", "n_run", "a_seq")})

    def check(out, b, slot):
        for k in ("xs", "acts", "costs", "omega", "ic"):
            assert np.array_equal(out[k][:, slot], want[k], equal_nan=True), (k, slot)
        for k in ("loss", "status", "n_run", "a_seq"):
            assert np.array_equal(out[k][slot], want[k]), (k, slot)
        assert np.array_equal(b.get_a_seq()[slot], r["after"][0][0][e]) and np.array_equal(b.get_actions()[slot], r["after"][0][1][e]), slot

    alone = _batch(case, inp, [e])
    check(_sim(alone, case, inp, [e]), alone, 0)
    alone.close()
    envs = [e, 0, e, 3, e]
    five = _batch(case, inp, envs)
    out = _sim(five, case, inp, envs)
    for slot in (0, 2, 4):
        check(out, five, slot)
    five.close()
    # slot 0 inactive, slot 1 already stopped (status 1 at entry), slot 3 stops earlier, slot 4 later (never)
    envs = [3, 3, e, 0, 3]
    b = _batch(case, inp, envs)
    seq0 = b.get_a_seq()
    loss0, stat0 = np.array([7.0, 5.0, 0.0, 0.0, 0.0], np.float32), np.array([0, 1, 0, 0, 0], np.int32)
    out = _sim(b, case, inp, envs, active=[0, 1, 1, 1, 1], loss=loss0, status=stat0)
    check(out, b, 2)
    assert out["n_run"].tolist() == [-1, 0, 2, 1, T] and out["status"].tolist() == [0, 1, 2, 2, 0]
    assert out["loss"][0] == 7.0 and out["loss"][1] == 5.0  # neither is written
    for k in ("xs", "acts", "costs", "omega", "ic"):
        assert np.isnan(out[k][:, :2]).all(), k
    assert np.isnan(out["a_seq"][:2]).all() and np.array_equal(b.get_a_seq()[:2], seq0[:2])
    b.close()
    # a clone between two calls finishes as the original does
    b = _batch(case, inp)
    one = _sim(b, case, inp, range(case["B"]), 0, 1)
    twin = copy.deepcopy(b)
    x, y = (_sim(v, case, inp, range(case["B"]), 1, T, states=_carry(one, inp["st"]), loss=one["loss"], status=one["status"]) for v in (b, twin))
    for k in NAMES:
        assert np.array_equal(x[k], y[k], equal_nan=True), k
    assert np.array_equal(x["loss"], r["loss"]) and np.array_equal(b.get_a_seq(), twin.get_a_seq())
    b.close()
    twin.close()


# ------------------------------------------------------------------------------------------------ 6. plumbing
def test_t_launches_per_call_and_refusals_before_any_launch():
    L = _L()
    case = cases.BY_ID["part_map"]
    inp = _inputs(case)
    B, S, H, T = case["B"], case["S"], case["H"], case["T"]
    b = _batch(case, inp)
    b.ctx.profile(True)
    count = lambda: b.ctx.profile_get().get("amppi_kernel", (0.0, 0))[1]
    total = lambda: sum(v[1] for v in b.ctx.profile_get().values())
    r = _sim(b, case, inp, range(B))
    assert count() == T == total() and r["n_run"].tolist() == [1, 1, 2, 3]  # T launches whatever stops, no roll launch
    one = _batch(case, inp, [0])  # ... and whatever B: the lone environment stops in period 0
    one.ctx.profile(True)
    _sim(one, case, inp, [0])
    assert sum(v[1] for v in one.ctx.profile_get().values()) == T
    one.close()
    before = (b.get_a_seq(), b.get_actions())
    lib, FP, IP = L.load(), L.FP, __import__("ctypes").POINTER(__import__("ctypes").c_int)
    f = lambda a: np.ascontiguousarray(a, np.float32)
    st, params, plant = _sub(inp, range(B), 0, T)
    sp, pp, lp = f(st), f(params), f(plant)
    SENT = np.float32(-77.0)
    xs, ac_, co, om, ic, sq = (np.full(s, SENT, np.float32) for s in ((T, B, 4), (T, B, 2), (T, B, S), (T, B, S), (T, B), (B, H, 2)))
    loss, status, n_run = np.full(B, 3.0, np.float32), np.zeros(B, np.int32), np.full(B, -5, np.int32)
    P = lambda a: None if a is None else a.ctypes.data_as(FP)
    PI = lambda a: None if a is None else a.ctypes.data_as(IP)
    from dust_amd.backend import _episode_rules

    import ctypes as C

    def rules(**kw):
        d = dict(t0=0, warm_up=0, goal=cases.PART_GOAL, goal_radius=1.0, stop_on_crash=True)
        d.update(kw)
        ru = _episode_rules(4, d["t0"], d["warm_up"], d["goal"], d["goal_radius"], d["stop_on_crash"])
        return ru

    def call(states=sp, n=T, prm=pp, plt=lp, flags=0, roll=1, ru=rules(), so=xs, ao=ac_, ico=ic, lo=loss, stt=status, nr=n_run, h=b._h):
        return lib.dust_amppi_batch_simulate(h, P(states), n, P(prm), flags, roll, P(plt), None if ru is None else C.byref(ru), None, P(so), P(ao), P(co),
                                             P(om), P(ico), P(lo), PI(stt), PI(nr), P(sq))

    bad_goal = rules()
    bad_goal.goal[1] = float("nan")
    bad_status = np.array([0, 3, 0, 0], np.int32)
    refused = [(call(states=None), L.ERR_INVALID), (call(so=None), L.ERR_INVALID), (call(ao=None), L.ERR_INVALID), (call(n=0), L.ERR_INVALID),
               (call(n=4097), L.ERR_INVALID), (call(roll=0), L.ERR_INVALID), (call(h=None), L.ERR_INVALID),
               (call(ru=None), L.ERR_INVALID), (call(lo=None), L.ERR_INVALID), (call(stt=None), L.ERR_INVALID), (call(nr=None), L.ERR_INVALID),
               (call(ico=None), L.ERR_INVALID), (call(ru=rules(warm_up=1)), L.ERR_INVALID), (call(ru=rules(t0=-1)), L.ERR_INVALID),
               (call(ru=bad_goal), L.ERR_INVALID), (call(ru=rules(goal_radius=float("inf"))), L.ERR_INVALID), (call(stt=bad_status), L.ERR_INVALID),
               (call(flags=L.PTR_DEVICE), L.ERR_UNSUPPORTED), (call(flags=L.STORE_STATES), L.ERR_UNSUPPORTED),
               (call(flags=L.EPS_F16), L.ERR_UNSUPPORTED), (call(flags=L.STORE_F16), L.ERR_UNSUPPORTED)]
    for k, (got, want) in enumerate(refused):
        assert got == want, (k, got, want)
    assert count() == T == total()
    after = (b.get_a_seq(), b.get_actions())
    assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1], equal_nan=True)
    for v in (xs, ac_, co, om, ic, sq):
        assert (v == SENT).all()
    assert (loss == 3.0).all() and not status.any() and (n_run == -5).all()
    b.close()
    # stop_on_crash without an occupancy map; parameter rows without uncertain parameters
    c0 = cases.BY_ID["roll3"]
    i0 = _inputs(c0)
    b0 = _batch(c0, i0)
    b0.ctx.profile(True)
    with pytest.raises(L.DustError) as e:
        b0.simulate(i0["st"], 1, stop_on_crash=True)
    assert e.value.status == L.ERR_UNSUPPORTED
    with pytest.raises(L.DustError) as e:
        b0.simulate(i0["st"], 1, plant_params=np.ones((c0["B"], 1), np.float32))
    assert e.value.status == L.ERR_INVALID and sum(v[1] for v in b0.ctx.profile_get().values()) == 0
    b0.close()


def test_staging_and_record_caps_are_the_plain_episode_s():
    """2^28 values of staged parameter rows, or of records, per call: beyond either the call refuses with DUST_ERR_UNSUPPORTED and says to
    split the episode - before it reads the (here far too small) arrays, writes the in-out words or launches anything"""
    import ctypes as C

    from dust_amd import Context
    from dust_amd.backend import _episode_rules

    L = _L()
    s = ac.A("bound", "pendulum", 65536, 1, "extended", ("length", "mass"), 5)
    c = Context(**ac.context_kwargs(s))
    batch = c.amppi_batch(1)
    c.close()
    batch.ctx.profile(True)
    lib, FP, IP = L.load(), L.FP, C.POINTER(C.c_int)
    small, loss, status, n_run = np.zeros(16, np.float32), np.full(1, 3.0, np.float32), np.zeros(1, np.int32), np.full(1, -5, np.int32)
    P = small.ctypes.data_as(FP)
    ru = _episode_rules(2, 0, 0, (0.0, 0.0), 0.5, False)
    words = (loss.ctypes.data_as(FP), status.ctypes.data_as(IP), n_run.ctypes.data_as(IP))
    before = batch.get_a_seq()
    # 4096 periods x 65536 rows x 2 columns = 2^29 values to stage
    assert lib.dust_amppi_batch_simulate(batch._h, P, 4096, P, 0, 1, None, C.byref(ru), None, P, P, None, None, P, *words, None) == L.ERR_UNSUPPORTED
    assert "split the episode" in lib.dust_last_error().decode()
    # 2048 periods: 2^28 values to stage pass the first bound (it is "more than"); costs and omega records are 2 x 2^27 + ... values
    assert lib.dust_amppi_batch_simulate(batch._h, P, 2048, P, 0, 1, None, C.byref(ru), None, P, P, P, P, P, *words, None) == L.ERR_UNSUPPORTED
    assert "split the episode" in lib.dust_last_error().decode() and "record" in lib.dust_last_error().decode()
    assert batch.ctx.profile_get() == {} and np.array_equal(batch.get_a_seq(), before) and not small.any()
    assert loss[0] == 3.0 and status[0] == 0 and n_run[0] == -5
    batch.close()


# ------------------------------------------------------------------------------------------------ 7. the class, the driver, the example
def _particle_ctrl(B=4, S=64, H=8, mode="extended"):
    import torch.distributions as dist

    from dust_amd.controllers import BatchAMPPI
    from dust_amd.models import Particle

    model = Particle(**ac.PART_ENV, mass=2.0, uncertain_params=("mass",))
    model.params_dist = dist.Independent(dist.Uniform(torch.tensor([1.8]), torch.tensor([2.2])), 1)
    g = torch.Generator().manual_seed(3)
    ctrl = BatchAMPPI(B, model.observation_space, model.action_space, H, S, lambda_=50.0, a_cov=25.0 * torch.eye(2),
                      inst_cost_fn=model.default_inst_cost, term_cost_fn=model.default_term_cost, params_sampling=mode,
                      init_actions=0.5 * torch.randn(H, 2, generator=g), seeds=[5, 6, 7, 8][:B])
    ctrl.return_rollouts = False
    start = torch.tensor(cases.BY_ID["part_map"]["start"])
    true = torch.tensor([[2.8], [1.4], [2.4], [1.7]])
    return ctrl, model, start, true


def test_simulate_against_update_actions_and_roll_and_resume_across_a_stop():
    """the class against a deep copy driven by its own update_actions / roll with the rules on the host, fed the parameter rows the call
    drew (under one torch seed: T draws per active environment); then resume across the stops against the one call"""
    case = cases.BY_ID["part_map"]
    T, B, grid = 3, 4, cases.grid_of(case)
    ep, model, start, true = _particle_ctrl()
    ep.update_actions(model, start)  # (creates the device batch, so that the deep copies below carry one)
    ep.roll(1)
    ticks, pieces = copy.deepcopy(ep), copy.deepcopy(ep)
    kw = dict(goal=model.target, goal_radius=1.0, stop_on_crash=True, plant_params=true)
    torch.manual_seed(40)
    rows = torch.stack([torch.stack([model.dict_to_params(model.sample_params(ep._sample_shape)) for _ in range(B)]) for _ in range(T)])
    torch.manual_seed(40)
    res = ep.simulate(model, start, T, **kw)
    after = torch.rand(1)
    torch.manual_seed(40)
    for _ in range(T * B):
        model.sample_params(ep._sample_shape)
    assert torch.equal(torch.rand(1), after)  # the torch stream stands where T x B draws leave it
    assert res.status.tolist() == [2, 1, 2, 0] and res.n_run.tolist() == [1, 1, 2, 3] and res.t0 == T
    assert bool(torch.isinf(res.loss[[0, 2]]).all()) and bool(torch.isfinite(res.loss[[1, 3]]).all())
    on, x = np.ones(B, bool), start.clone()
    for t in range(T):
        c_t, _, _, o_t = ticks.update_actions(model, x, active=on.tolist(), params=rows[t])
        first = ticks.a_seq[:, 0]
        ticks.roll(1, active=on.tolist())
        for e in np.nonzero(on)[0]:
            assert torch.equal(c_t[e], res.costs[t, e]) and torch.equal(o_t[e], res.omega[t, e]) and torch.equal(first[e], res.actions[t, e]), (t, e)
            x[e] = res.states[t, e]
        stat = cases.apply_rules(case, x.numpy(), grid)
        on &= stat == 0
    assert torch.equal(ep.a_seq, ticks.a_seq)
    one = pieces.simulate(model, start, 1, params=rows[:1], **kw)
    x = start.clone()
    for e in range(B):
        x[e] = one.states[0, e]
    two = pieces.simulate(model, x, T - 1, params=rows[1:], resume=one, **kw)
    assert two.t0 == T and torch.equal(two.loss, res.loss) and torch.equal(two.status, res.status) and two.n_run.tolist() == [0, 0, 1, 2]
    assert torch.equal(pieces.a_seq, ep.a_seq)


def test_run_particle_episodes_with_a_batch_amppi_and_a_load():
    from dust_amd.utils.simulations import run_particle_episodes

    ctrl, model, start, true = _particle_ctrl()
    twin = copy.deepcopy(ctrl)
    steps, load = 8, 0.5
    torch.manual_seed(7)
    loss = run_particle_episodes(start, model, None, ctrl, warm_up=30, load=load, steps=steps, plant_params=true)
    kw = dict(goal=model.target, goal_radius=1.0, stop_on_crash=True)
    torch.manual_seed(7)
    one = twin.simulate(model, start, steps // 4, plant_params=true, **kw)
    x = start.clone()
    for e in range(4):
        if one.n_run[e] > 0:
            x[e] = one.states[one.n_run[e] - 1, e]
    two = twin.simulate(model, x, steps - steps // 4, plant_params=true + load, resume=one, **kw)
    assert torch.equal(loss, two.loss) and bool(torch.isinf(loss[[0, 2]]).all()) and bool(torch.isfinite(loss[[1, 3]]).all())
    assert torch.equal(ctrl.a_seq, twin.a_seq)


def test_example_runs_tiny():
    path = os.path.join(ROOT, "examples", "amppi_sim_example.py")
    spec = importlib.util.spec_from_file_location("amppi_sim_example", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    losses, status, n_run = mod.run(quiet=True, **mod.TINY)
    B = mod.TINY["n_envs"]
    assert tuple(losses.shape) == (B,) == tuple(status.shape) == tuple(n_run.shape)
    assert bool((torch.isinf(losses) == (status == 2)).all()) and bool((n_run >= 1).all())
