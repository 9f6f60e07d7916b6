"""Per-environment hyper-parameters in the batched SVMPC tick and its episodes (dust_svmpc_batch_set_hyper / _get_hyper, csrc/svmpc_batch.hpp
svmpc_sweep_kernel, csrc/svmpc_episode.hpp svmpc_sweep_episode_kernel, `SvmpcBatch.set_hyper`, `BatchSVMPC.set_hyper`): lr, alpha,
temperature, sigma_a / chol_a, sigma_p and weighted_prior of every environment from its own row.  The feature adds no arithmetic - a
workgroup runs the uniform kernels' text on its own copy of the arguments - so every comparison below is np.array_equal, bit for bit
(item 5 alone holds the reference's fixtures at their stored tolerances).

1. environment b of a batch with rows against a one-environment batch of a prototype built with row b's values;
2. rows equal to the prototype's in every environment against the same batch without rows: the new instances against the old;
3. power: one field of one row changed shows in that environment - at the getter named for the field - and nowhere else;
4. an environment computes the same alone, in slots 0 / 2 / 4 of five, beside inactive neighbours and from a clone; set_hyper(None)
   returns the batch to the no-rows result; get_hyper round-trips;
5. the reference's cart-pole tick fixtures in the middle slot of three, among neighbours with other rows;
6. episodes: against T ticks of a clone, against the uniform one-environment batch's episode, two chained against one;
7. one launch per call, the refusals before any launch, invalid rows;
8. `BatchSVMPC.set_hyper` against B one-environment objects, a deep copy mid-loop, a rebuilt batch, the example.
"""
import copy
import functools
import importlib.util
import os

import numpy as np
import pytest
import torch

import svmpc_sweep_cases as cases
from helpers import elemerr, relerr

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GETTERS = ("THETA", "PRIOR_MEANS", "PRIOR_MIX", "A_MAT", "COSTS", "SCORE", "PHI", "LOG_L", "LOG_P", "A_MIX")


def _L():
    from dust_amd import _lib

    return _lib


def _records(b, actions=False):
    L = _L()
    return {n: b.get(getattr(L, "SVB_" + n)) for n in GETTERS + (("ACTIONS",) if actions else ())}


def _grid(case):
    if case["family"] == "particle":
        from oracle import grid_4x4_map

        return grid_4x4_map()
    return None


def _batch(case, inp, envs, row=None, rows=None):
    """a batch whose slot k holds environment envs[k]'s inputs; `row`: the prototype is built with these values; `rows`: set_hyper"""
    from dust_amd import Context

    L = _L()
    envs = list(envs)
    c = Context(grid=_grid(case), **cases.context_kwargs(case, row))
    b = c.svmpc_batch(len(envs), seeds=[inp["seeds"][e] for e in envs])
    c.close()
    b.set(L.SVB_THETA, inp["th"][envs])
    b.set(L.SVB_PRIOR_MEANS, inp["mu"][envs])
    b.set(L.SVB_A_MAT, inp["am"][envs])
    if rows is not None:
        b.set_hyper(cases.stack(rows))
    return b


def _ticks(case, b, inp, envs, ext_noise, active=None, ticks=3, clone_after=None):
    """three ticks of the case's n_steps -> per tick the records, a_seq and p_weights (and the same of a clone taken after a tick)"""
    envs = list(envs)
    out, twin, out_twin = [], None, []
    for t in range(ticks):
        n = case["iters"][t]
        kw = dict(eps=np.ascontiguousarray(inp["eps"][t][envs]) if ext_noise else None,
                  params=None if inp["params"][t] is None else np.ascontiguousarray(inp["params"][t][envs]), active=active, keep_actions=True)
        a_seq, pw = b.tick(inp["st"][envs], n, **kw)
        out.append(dict(_records(b, actions=True), a_seq=a_seq, pw=pw))
        if twin is not None:
            a2, p2 = twin.tick(inp["st"][envs], n, **kw)
            out_twin.append(dict(_records(twin, actions=True), a_seq=a2, pw=p2))
        if clone_after == t:
            twin = b.clone()
    if twin is not None:
        twin.close()
    return out, out_twin


def _same(got, slot, want, wslot=0, what=""):
    for t, (g, w) in enumerate(zip(got, want)):
        for k, v in w.items():
            assert np.array_equal(g[k][slot], v[wslot]), (what, t, k)


@functools.lru_cache(maxsize=None)
def _sweep(cid, ext_noise):
    """the case's batch with its rows: three ticks, recorded once"""
    case = cases.BY_ID[cid]
    inp = cases.env_inputs(case)
    b = _batch(case, inp, range(case["B"]), rows=cases.env_rows(case))
    out, _ = _ticks(case, b, inp, range(case["B"]), ext_noise)
    b.close()
    return inp, out


# ------------------------------------------------------------------------------------------------ 1. against a uniform batch
@pytest.mark.parametrize("ext_noise", [True, False], ids=["recorded", "device"])
@pytest.mark.parametrize("cid", cases.IDS)
def test_environment_equals_a_uniform_batch_of_its_row(cid, ext_noise):
    case = cases.BY_ID[cid]
    inp, got = _sweep(cid, ext_noise)
    rows = cases.env_rows(case)
    for e in range(case["B"]):
        one = _batch(case, inp, [e], row=rows[e])
        want, _ = _ticks(case, one, inp, [e], ext_noise)
        one.close()
        _same(got, e, want, what=(cid, e))
    assert np.isfinite(got[-1]["THETA"]).all() and np.isfinite(got[-1]["pw"]).all()
    if case["N"] * case["H"] > 1:  # the rows matter: environments 0 and 1 would otherwise differ by their inputs alone
        assert not np.array_equal(got[0]["THETA"][0], got[0]["THETA"][1])


# ------------------------------------------------------------------------------------------------ 2. the new instances against the old
@pytest.mark.parametrize("ext_noise", [True, False], ids=["recorded", "device"])
@pytest.mark.parametrize("cid", cases.IDS)
def test_prototype_rows_equal_no_rows(cid, ext_noise):
    case = cases.BY_ID[cid]
    inp, B = cases.env_inputs(case), case["B"]
    plain = _batch(case, inp, range(B))
    want, _ = _ticks(case, plain, inp, range(B), ext_noise)
    swept = _batch(case, inp, range(B))
    proto = swept.get_hyper()  # without rows: B times the prototype's values
    for k, v in cases.stack([cases.base_row(case)] * B).items():
        assert np.array_equal(proto[k], v.reshape(proto[k].shape)), k
    swept.set_hyper(proto)
    swept.ctx.profile(True)
    got, _ = _ticks(case, swept, inp, range(B), ext_noise)
    assert swept.ctx.profile_get()["svmpc_batch_kernel"][1] == 3
    plain.close()
    swept.close()
    for e in range(B):
        _same(got, e, want, wslot=e, what=(cid, e))


# ------------------------------------------------------------------------------------------------ 3. power
@pytest.mark.parametrize("field", list(cases.VARIANTS))
@pytest.mark.parametrize("cid", ["pend", "part"])
def test_one_field_of_one_row_shows_there_and_nowhere_else(cid, field):
    case = cases.BY_ID[cid]
    inp, base = _sweep(cid, True)
    rows = cases.env_rows(case)
    change, where = cases.VARIANTS[field]
    var = list(rows)
    var[2] = change(rows[2])
    assert not cases.row_equal(var[2], rows[2])
    b = _batch(case, inp, range(case["B"]), rows=var)
    got, _ = _ticks(case, b, inp, range(case["B"]), True)
    b.close()
    for e in (0, 1, 3, 4):
        _same(got, e, base, wslot=e, what=(cid, field, e))
    shows = [k for k in GETTERS if any(not np.array_equal(g[k][2], w[k][2]) for g, w in zip(got, base))]
    print(cid, field, "shows in", shows)
    assert any(k in shows for k in where), (field, where, shows)


# ------------------------------------------------------------------------------------------------ 4. independence
@pytest.mark.parametrize("ext_noise", [True, False], ids=["recorded", "device"])
@pytest.mark.parametrize("cid", ["pend", "part"])
def test_an_environment_does_not_depend_on_its_batch(cid, ext_noise):
    case = cases.BY_ID[cid]
    inp, full = _sweep(cid, ext_noise)
    rows = cases.env_rows(case)
    e = 3  # the two-softmax row
    alone = _batch(case, inp, [e], rows=[rows[e]])
    want, _ = _ticks(case, alone, inp, [e], ext_noise)
    alone.close()
    _same(full, e, want, what="in its own slot")
    envs = [e, 0, e, 4, e]  # slots 0 / 2 / 4 of five, other neighbours
    five = _batch(case, inp, envs, rows=[rows[k] for k in envs])
    got, twin = _ticks(case, five, inp, envs, ext_noise, clone_after=0)
    five.close()
    for slot in (0, 2, 4):
        _same(got, slot, want, what=("slot", slot))
    for t, w in enumerate(got[1:]):  # the clone taken after the first tick carries the rows: it continues identically, every slot
        for k, v in w.items():
            assert np.array_equal(twin[t][k], v), ("clone", t, k)
    # beside inactive neighbours, which keep everything
    L = _L()
    envs = [0, e, 4]
    three = _batch(case, inp, envs, rows=[rows[k] for k in envs])
    keep = [three.get(w) for w in (L.SVB_THETA, L.SVB_PRIOR_MEANS, L.SVB_PRIOR_MIX, L.SVB_A_MAT)]
    got, _ = _ticks(case, three, inp, envs, ext_noise, active=np.array([0, 1, 0], np.uint8))
    _same(got, 1, want, what="beside sleepers")
    assert np.isnan(got[-1]["a_seq"][[0, 2]]).all() and np.isnan(got[-1]["pw"][[0, 2]]).all()
    for w, v in zip((L.SVB_THETA, L.SVB_PRIOR_MEANS, L.SVB_PRIOR_MIX, L.SVB_A_MAT), keep):
        assert np.array_equal(three.get(w)[[0, 2]], v[[0, 2]])
    three.close()


@pytest.mark.parametrize("cid", ["pend", "part"])
def test_set_hyper_null_returns_to_the_prototype_and_get_hyper_round_trips(cid):
    case = cases.BY_ID[cid]
    inp, B = cases.env_inputs(case), case["B"]
    rows = cases.stack(cases.env_rows(case))
    plain = _batch(case, inp, range(B))
    want, _ = _ticks(case, plain, inp, range(B), False)
    plain.close()
    b = _batch(case, inp, range(B))
    before = {w: b.get(getattr(_L(), "SVB_" + w)) for w in ("THETA", "PRIOR_MEANS", "PRIOR_MIX", "A_MAT")}
    b.set_hyper(rows)
    back = b.get_hyper()
    for k, v in rows.items():
        assert np.array_equal(back[k], v.reshape(back[k].shape)), k
    assert back["lr"].dtype == np.float64 and back["alpha"].dtype == np.float32 and back["sigma_p"].shape == (B, cases.family(case)["da"])
    for w, v in before.items():  # set_hyper touches nothing else
        assert np.array_equal(b.get(getattr(_L(), "SVB_" + w)), v), w
    b.set_hyper(None)
    got, _ = _ticks(case, b, inp, range(B), False)
    for e in range(B):
        _same(got, e, want, wslot=e)
    b.set_hyper(rows)  # ... and rows set between two ticks take over from there: the Philox position and the optimiser state stay
    twin = b.clone()
    assert all(np.array_equal(v, twin.get_hyper()[k]) for k, v in b.get_hyper().items())
    st = inp["st"]
    kw = dict(params=inp["params"][0])
    a1, p1 = b.tick(st, case["iters"][0], **kw)
    a2, p2 = twin.tick(st, case["iters"][0], **kw)
    assert np.array_equal(a1, a2) and np.array_equal(p1, p2) and not np.array_equal(a1, want[0]["a_seq"])
    b.close()
    twin.close()


# ------------------------------------------------------------------------------------------------ 5. the reference's fixtures
@pytest.mark.parametrize("name", ["tick_k1_sgd", "tick_k1_adam"])
def test_cartpole_ticks_vs_reference_among_differing_neighbours(golden, name):
    """tests/test_gpu_svmpc_batch.py test_cartpole_ticks_vs_reference_in_the_middle_slot with rows: the middle row is the fixture's own
    (the prototype's values), the neighbours' rows differ in every field and get other noise.  A neighbour's row must not leak."""
    from cartpole_cases import TICK_BY_TAG, controller_kwargs, twin
    from dust_amd import Context

    L = _L()
    g, s = golden("cartpole_" + name), TICK_BY_TAG[name]
    K, N = int(g["K"]), s["N"]
    kw = dict(kernel=s["kernel"], optimizer=s["opt"], lr=s["lr"], alpha=s["alpha"], temperature=4.0, chol_a=float(g["chol_a"]), a_pre=float(g["a_pre"]),
              sigma_a=float(g["sigma"]), sigma_p=float(g["sigma"]))
    rng = np.random.default_rng(1)
    c = Context(**controller_kwargs(s, **kw))
    c.set_theta(g["theta0"])
    c.set_prior(g["mu0"], np.ones(N, np.float32))
    c.set_a_mat(g["theta0"])
    states = np.stack([g["state"]] * 3)

    def three(x, noise=False):
        x = np.asarray(x, np.float32)
        side = rng.standard_normal(x.shape).astype(np.float32) if noise else x
        return np.stack([side, x, side])

    def with_rows(b):
        h = b.get_hyper()  # [3] times the fixture's own values
        own = {k: v[1].copy() for k, v in h.items()}
        h["lr"][[0, 2]] *= (3.0, 0.25)
        h["alpha"][[0, 2]] *= np.float32(2.0)
        h["temperature"][[0, 2]] *= (np.float32(0.5), np.float32(3.0))
        for k in ("sigma_a", "chol_a", "sigma_p"):
            h[k][[0, 2]] *= np.float32(1.5)
        h["weighted_prior"][[0, 2]] = 1
        b.set_hyper(h)
        assert all(np.array_equal(b.get_hyper()[k][1], v) for k, v in own.items())
        return b

    errs = {}
    b = with_rows(c.svmpc_batch(3))
    for k in range(K):
        b.optimize(states, 1, eps=three(g["eps"][k][None], noise=True), params=three(g["params"][k][None]))
        for q, v in (("costs", b.get(L.SVB_COSTS)[1]), ("theta_after", b.get(L.SVB_THETA)[1])):
            errs["%s[%d]" % (q, k)] = (min(elemerr(v, g[q][k]), elemerr(v, g[q + "_f64"][k])), float(g["tol_" + q]))
    assert elemerr(g["costs_off"], b.get(L.SVB_COSTS)[1]) >= 9 * float(g["tol_costs"])
    b.close()
    b = with_rows(c.svmpc_batch(3))
    b.set(L.SVB_THETA, three(g["theta_in"][K - 1]))
    b.set(L.SVB_A_MAT, three(g["a_mat"][K - 2] if K > 1 else g["theta0"]))
    b.optimize(states, 1, eps=three(g["eps"][K - 1][None], noise=True), params=three(g["params"][K - 1][None]))
    b.set(L.SVB_THETA, three(g["theta_after"][K - 1]))
    a_seq, pw = b.forward()
    for q, v in (("log_l", b.get(L.SVB_LOG_L)[1]), ("log_p", b.get(L.SVB_LOG_P)[1]), ("p_weights", pw[1])):
        errs[q] = (min(elemerr(v, g[q]), elemerr(v, twin(g, q))), float(g["tol_" + q]))
    assert int(np.argmax(pw[1])) == int(np.argmax(g["p_weights"]))
    assert np.array_equal(a_seq[1], g["a_seq"])
    assert relerr(b.get(L.SVB_THETA)[1], g["theta_rolled"]) < 1e-6
    assert relerr(b.get(L.SVB_PRIOR_MEANS)[1], g["prior_means"]) < 1e-6 and elemerr(b.get(L.SVB_PRIOR_MIX)[1], g["prior_probs"]) < 1e-5
    assert not np.array_equal(b.get(L.SVB_PRIOR_MIX)[0], b.get(L.SVB_PRIOR_MIX)[1])  # (the neighbours' priors are weighted)
    b.close()
    c.close()
    print(name + " " + "  ".join("%s %.1e/%.1e" % (q, e, t) for q, (e, t) in errs.items()))
    for q, (e, t) in errs.items():
        assert e < t, (name, q, e, t)


# ------------------------------------------------------------------------------------------------ 6. episodes
def _ep_args(case, inp, envs, t0=0, t1=None):
    envs = list(envs)
    p = inp["ep_params"]
    return (None if p is None else np.ascontiguousarray(p[t0:t1][:, envs]), None if inp["plant"] is None else inp["plant"][envs])


@functools.lru_cache(maxsize=None)
def _episode(cid):
    """the case's episode with rows and, on a clone taken before it, its T ticks fed the recorded states; then one further tick on both"""
    case = cases.BY_ID[cid]
    T, n, B = cases.T_EPISODE, case["iters"][0], case["B"]
    inp = cases.env_inputs(case)
    b = _batch(case, inp, range(B), rows=cases.env_rows(case))
    twin = b.clone()
    params, plant = _ep_args(case, inp, range(B), 0, T)
    b.ctx.profile(True)
    xs, acts, pw, a_seq = b.episode(inp["st"], T, n, params, plant)
    launches = b.ctx.profile_get()["svmpc_batch_kernel"][1]
    ticks, x = [], inp["st"]
    for t in range(T):
        ticks.append(twin.tick(x, n, params=None if params is None else params[t]))
        x = xs[t]
    out = dict(inp=inp, xs=xs, acts=acts, pw=pw, a_seq=a_seq, ticks=ticks, after=(_records(b), _records(twin)), launches=launches)
    extra = None if inp["ep_params"] is None else np.ascontiguousarray(inp["ep_params"][T])
    out["further"] = (b.tick(xs[-1], n, params=extra), twin.tick(xs[-1], n, params=extra), _records(b), _records(twin))
    b.close()
    twin.close()
    return out


@pytest.mark.parametrize("cid", cases.EPISODE_IDS)
def test_episode_with_rows_equals_its_periods(cid):
    case, r = cases.BY_ID[cid], _episode(cid)
    T, B, f = cases.T_EPISODE, case["B"], cases.family(case)
    assert r["launches"] == 1
    assert r["xs"].shape == (T, B, f["ds"]) and r["acts"].shape == (T, B, f["da"]) and r["pw"].shape == (T, B, case["N"])
    assert np.isfinite(r["xs"]).all() and np.isfinite(r["acts"]).all()
    for t, (a_t, pw_t) in enumerate(r["ticks"]):
        assert np.array_equal(a_t[:, 0], r["acts"][t]), t
        assert np.array_equal(pw_t, r["pw"][t]), t
    assert np.array_equal(r["ticks"][-1][0], r["a_seq"])
    for k in GETTERS:
        assert np.array_equal(r["after"][0][k], r["after"][1][k]), k
    (a1, p1), (a2, p2), g1, g2 = r["further"]
    assert np.array_equal(a1, a2) and np.array_equal(p1, p2)
    for k in GETTERS:
        assert np.array_equal(g1[k], g2[k]), k


@pytest.mark.parametrize("cid", cases.EPISODE_IDS)
def test_episode_environment_equals_the_uniform_batch_of_its_row(cid):
    case, r = cases.BY_ID[cid], _episode(cid)
    T, n, inp = cases.T_EPISODE, case["iters"][0], r["inp"]
    rows = cases.env_rows(case)
    for e in range(case["B"]):
        one = _batch(case, inp, [e], row=rows[e])
        params, plant = _ep_args(case, inp, [e], 0, T)
        xs, acts, pw, a_seq = one.episode(inp["st"][[e]], T, n, params, plant)
        got = _records(one)
        one.close()
        assert np.array_equal(xs[:, 0], r["xs"][:, e]) and np.array_equal(acts[:, 0], r["acts"][:, e]), e
        assert np.array_equal(pw[:, 0], r["pw"][:, e]) and np.array_equal(a_seq[0], r["a_seq"][e]), e
        for k in GETTERS:
            assert np.array_equal(got[k][0], r["after"][0][k][e]), (e, k)


@pytest.mark.parametrize("cid", cases.EPISODE_IDS)
def test_two_episodes_with_rows_concatenate(cid):
    case, r = cases.BY_ID[cid], _episode(cid)
    T, n, B, inp = cases.T_EPISODE, case["iters"][0], case["B"], r["inp"]
    b = _batch(case, inp, range(B), rows=cases.env_rows(case))
    p1, plant = _ep_args(case, inp, range(B), 0, 1)
    p2, _ = _ep_args(case, inp, range(B), 1, T)
    x1, a1, w1, _ = b.episode(inp["st"], 1, n, p1, plant)
    x2, a2, w2, s2 = b.episode(x1[-1], T - 1, n, p2, plant)
    got = _records(b)
    b.close()
    assert np.array_equal(np.concatenate((x1, x2)), r["xs"]) and np.array_equal(np.concatenate((a1, a2)), r["acts"])
    assert np.array_equal(np.concatenate((w1, w2)), r["pw"]) and np.array_equal(s2, r["a_seq"])
    for k in GETTERS:
        assert np.array_equal(got[k], r["after"][0][k]), k


# ------------------------------------------------------------------------------------------------ 7. plumbing
def test_one_launch_per_call_and_invalid_rows():
    L = _L()
    case = cases.BY_ID["pend"]
    inp, B = cases.env_inputs(case), case["B"]
    rows = cases.stack(cases.env_rows(case))
    b = _batch(case, inp, range(B))
    b.set_hyper(rows)
    b.ctx.profile(True)
    count = lambda: b.ctx.profile_get().get("svmpc_batch_kernel", (0.0, 0))[1]
    total = lambda: sum(v[1] for v in b.ctx.profile_get().values())
    st, p = inp["st"], inp["params"]
    b.optimize(st, case["iters"][0], params=p[0])
    assert count() == 1 == total()
    b.forward()
    assert count() == 2 == total()
    b.tick(st, case["iters"][1], params=p[1])
    assert count() == 3 == total()
    params, plant = _ep_args(case, inp, range(B), 0, 2)
    b.episode(st, 2, case["iters"][0], params, plant)
    assert count() == 4 == total()
    before = _records(b)
    lib = L.load()
    assert lib.dust_svmpc_batch_get(b._h, 11, np.zeros(4, np.float32).ctypes.data_as(L.FP)) == L.ERR_INVALID  # the rows have getters of their own

    def bad(field, value, env=3, col=None):
        r = {k: v.copy() for k, v in rows.items()}
        if col is None:
            r[field][env] = value
        else:
            r[field][env, col] = value
        return r

    invalid = [bad("lr", np.nan), bad("lr", 0.0), bad("lr", np.inf), bad("alpha", 0.0), bad("alpha", np.nan), bad("temperature", -1.0),
               bad("temperature", np.inf), bad("sigma_a", -1.0, col=0), bad("chol_a", 0.0, col=0), bad("sigma_p", np.nan, col=0),
               bad("sigma_p", -1.0, col=0), bad("weighted_prior", 2), bad("weighted_prior", -1)]
    for r in invalid:
        with pytest.raises(L.DustError) as e:
            b.set_hyper(r)
        assert e.value.status == L.ERR_INVALID
        back = b.get_hyper()
        for k, v in rows.items():
            assert np.array_equal(back[k], v.reshape(back[k].shape)), k
    assert lib.dust_svmpc_batch_get_hyper(b._h, None) == L.ERR_INVALID and lib.dust_svmpc_batch_set_hyper(None, None) == L.ERR_INVALID
    assert count() == 4 == total()
    for k in GETTERS:
        assert np.array_equal(_records(b)[k], before[k]), k
    b.close()


def test_dual_loop_and_navigation_cost_are_refused_before_any_launch():
    import svmpc_episode_cases as ec
    from dust_amd import Context, MpfContext

    L = _L()
    case = cases.BY_ID["pend"]
    inp, B = cases.env_inputs(case), case["B"]
    rows = cases.stack(cases.env_rows(case))
    b = _batch(case, inp, range(B))
    rng = np.random.default_rng(3)
    x = (1.0 + 0.1 * rng.standard_normal((B, 16, 2))).astype(np.float32)
    m = MpfContext(x[0], inp["st"][0], model="pendulum", uncertain_params=("length", "mass"), obs_std=0.2, lr=1e-3, init_bw=0.05, optimizer="SGD",
                   log_space=False, dt=0.05)
    mb = m.batch(B)
    m.close()
    mb.set_particles(x)
    mb.set_obs(inp["st"])
    n = case["iters"][0]
    b.tick(inp["st"], n, params=inp["params"][0])  # (getters to keep)
    b.set_hyper(rows)
    b.ctx.profile(True)
    total = lambda: sum(v[1] for v in b.ctx.profile_get().values())
    before, filt, stats = _records(b), mb.get_particles(), mb.stats()
    keys = np.arange(1, B + 1, dtype=np.uint64)
    with pytest.raises(L.DustError, match="per-environment hyper-parameters") as e:
        b.dual_tick(mb, inp["st"], np.zeros((B, 1), np.float32), n_steps=n, mpf_steps=2, mpf_bw=0.05, seeds=keys)
    assert e.value.status == L.ERR_UNSUPPORTED
    with pytest.raises(L.DustError, match="per-environment hyper-parameters") as e:
        b.dual_episode(mb, inp["st"], 2, n, np.zeros((B, 1), np.float32), mpf_steps=2, mpf_bw=0.05, seeds=np.stack([keys, keys + 7]))
    assert e.value.status == L.ERR_UNSUPPORTED
    assert total() == 0 and mb.stats() == stats and np.array_equal(mb.get_particles(), filt)
    for k in GETTERS:
        assert np.array_equal(_records(b)[k], before[k]), k
    b.set_hyper(None)  # without rows the dual tick runs as before
    a_seq, _, _, _ = b.dual_tick(mb, inp["st"], None, n_steps=n, mpf_steps=2, mpf_bw=0.05, seeds=keys)
    assert np.isfinite(a_seq).all() and b.ctx.profile_get()["svmpc_batch_kernel"][1] == 1
    b.close()
    mb.close()
    # a navigation-cost prototype: every call of the batch while rows are set
    skid = cases.BY_ID["skid"]
    inp = cases.env_inputs(skid)
    c = Context(grid=ec.nav_map(), **dict(cases.context_kwargs(skid), **ec.NAV))
    nb = c.svmpc_batch(skid["B"], seeds=inp["seeds"])
    c.close()
    nb.set(L.SVB_THETA, inp["th"])
    nb.set(L.SVB_A_MAT, inp["am"])
    nb.tick(inp["st"], 1, params=inp["params"][1])
    nb.set_hyper(cases.stack(cases.env_rows(skid)))
    nb.ctx.profile(True)
    before = _records(nb)
    params, plant = _ep_args(skid, inp, range(skid["B"]), 0, 1)
    calls = (lambda: nb.optimize(inp["st"], 1, params=inp["params"][1]), lambda: nb.forward(), lambda: nb.tick(inp["st"], 1, params=inp["params"][1]),
             lambda: nb.episode(inp["st"], 1, skid["iters"][0], params, plant))
    for call in calls:
        with pytest.raises(L.DustError, match="navigation cost") as e:
            call()
        assert e.value.status == L.ERR_UNSUPPORTED
    assert sum(v[1] for v in nb.ctx.profile_get().values()) == 0
    for k in GETTERS:
        assert np.array_equal(_records(nb)[k], before[k]), k
    nb.set_hyper(None)
    nb.tick(inp["st"], 1, params=inp["params"][1])
    assert sum(v[1] for v in nb.ctx.profile_get().values()) == 1
    nb.close()


# ------------------------------------------------------------------------------------------------ 8. the class
def _mirror(n_envs, lr=0.25, alpha=1.0, temperature=1.0, prior_sigma=2.0, ctrl_sigma=2.0, weighted_prior=False, seeds=None, N=3, S=16, H=6, M=3):
    """the hyper-parameters travel as the tuning scripts pass them: into the optimiser, the likelihood, MultiDISCO and the prior"""
    from dust_amd.controllers import MultiDISCO
    from dust_amd.costs import PendulumQuadCos
    from dust_amd.inference import BatchSVMPC, ExponentiatedUtility, get_gmm
    from dust_amd.kernels import RBFKernel
    from dust_amd.models import PendulumModel

    model, cost = PendulumModel(uncertain_params=("length", "mass")), PendulumQuadCos()
    ctrl = MultiDISCO(model.observation_space, model.action_space, H, N, S, temperature=temperature, a_cov=ctrl_sigma ** 2 * torch.eye(1),
                      inst_cost_fn=cost.inst_cost, term_cost_fn=cost.term_cost, params_sampling=True, params_samples=M, seed=0)
    g = torch.Generator().manual_seed(3)
    mu = torch.randn(N, H, 1, generator=g)
    th = mu + 2 * torch.randn(N, H, 1, generator=g)
    ctrl.a_mat = th.clone()
    prior = get_gmm(mu, torch.ones(N), prior_sigma ** 2 * torch.eye(1))
    lik = ExponentiatedUtility(alpha=alpha, n_samples=S, controller=ctrl, model=model)
    return BatchSVMPC(n_envs, init_particles=th, prior=prior, likelihood=lik, kernel=RBFKernel(), n_particles=N, n_steps=2,
                      optimizer_class=torch.optim.SGD, lr=lr, weighted_prior=weighted_prior, seeds=seeds)


# (sigmas whose squares are exact in fp32: a covariance sigma^2 I then gives back sigma, as the rows carry it)
TRIALS = dict(lr=[0.25, 1.0, 0.5, 2.0], alpha=[1.0, 0.5, 2.0, 4.0], temperature=[1.0, 2.0, 1.5, 0.25], prior_sigma=[2.0, 0.5, 1.5, 4.0],
              ctrl_sigma=[2.0, 1.5, 0.75, 2.5], weighted_prior=[False, True, False, True])


def test_batch_svmpc_set_hyper_against_B_objects():
    """one BatchSVMPC of B environments with rows against B BatchSVMPC(1, ...) objects built with those hyper-parameters, under one torch
    seed (the B objects draw their dynamics samples in environment order, as the batch does); a deep copy after the first period; then a
    rebuilt batch (another parameter distribution's event shape changes the configuration) keeps its rows"""
    import torch.distributions as dist

    B = 4
    pd = dist.Independent(dist.Uniform(torch.tensor([0.8, 0.8]), torch.tensor([1.2, 1.2])), 1)
    seeds = [50 + b for b in range(B)]
    sweep = _mirror(B, seeds=seeds)
    sweep.set_hyper(**{k: torch.tensor(v) if k == "alpha" else v for k, v in TRIALS.items()})  # (before the batch exists: kept on the host)
    assert sweep._batch is None
    h = sweep.hyper
    assert np.array_equal(h["lr"], np.array(TRIALS["lr"])) and np.array_equal(h["sigma_a"][:, 0], np.array(TRIALS["ctrl_sigma"], np.float32))
    assert np.array_equal(h["chol_a"], h["sigma_a"]) and np.array_equal(h["weighted_prior"], [0, 1, 0, 1])
    lone = [_mirror(1, seeds=[seeds[b]], **{k: v[b] for k, v in TRIALS.items()}) for b in range(B)]
    states = torch.tensor([[3.0, 0.0], [2.5, 0.2], [3.4, -0.1], [2.9, 0.3]])
    for t in range(3):
        torch.manual_seed(40 + t)
        a_b, pw_b = sweep.tick(states, pd)
        torch.manual_seed(40 + t)
        outs = [lone[b].tick(states[b:b + 1], pd) for b in range(B)]
        for b in range(B):
            assert torch.equal(a_b[b], outs[b][0][0]) and torch.equal(pw_b[b], outs[b][1][0]), (t, b)
            assert torch.equal(sweep.theta[b], lone[b].theta[0]), (t, b)
        if t == 0:
            sweep, lone = copy.deepcopy(sweep), [copy.deepcopy(o) for o in lone]
            got = sweep.hyper
            assert all(np.array_equal(got[k], h[k]) for k in h)
    assert len({tuple(a_b[b].reshape(-1).tolist()) for b in range(B)}) == B
    # a rebuilt batch: the rows survive
    old = sweep._batch
    sweep.likelihood.controller._seed = 1  # (part of the configuration key)
    torch.manual_seed(50)
    sweep.tick(states, pd)
    assert sweep._batch is not old
    got = sweep.hyper
    assert all(np.array_equal(got[k], h[k]) for k in h)
    sweep.set_hyper()
    back = sweep.hyper
    assert np.array_equal(back["lr"], np.full(B, 0.25)) and not back["weighted_prior"].any()


def test_example_runs_tiny():
    path = os.path.join(ROOT, "examples", "svmpc_sweep_example.py")
    spec = importlib.util.spec_from_file_location("svmpc_sweep_example", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    cost, rows = mod.run(quiet=True, **mod.TINY)
    B = mod.TINY["n_envs"]
    assert tuple(cost.shape) == (B,) and bool(torch.isfinite(cost).all()) and len(set(cost.tolist())) == B
    assert np.array_equal(rows["temperature"], (1.0 / rows["alpha"]).astype(np.float32)) and len(set(rows["lr"].tolist())) == B
