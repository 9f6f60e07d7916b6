"""The skid-steer navigation cost in the batched SVMPC tick and its dual loop (csrc/svmpc_batch.hpp svmpc_skid_nav_batch_kernel and
svmpc_skid_nav_prior_batch_kernel; dust_svmpc_batch_*, dust_svmpc_dual_batch_tick, `BatchSVMPC`, `BatchDualSVMPC`): the quadratic family
plus w_obs on every occupied cell of ONE map shared by the B environments.

1. the reference, through the navigation fixtures (tests/golden/skid_nav_<tag>.npz, the scenarios of tests/skid_nav_cases.py) in the middle
   slot of three, at the fixtures' own stored tolerances and held away from every `costs_off_*` variant;
2. against a lone context on the same inputs, first-divergence form (test_gpu_svmpc_batch.py test_batch_equals_a_lone_context and its
   tolerances: costs and log_p 2e-5 element-wise, what lies downstream 5e-4, p_weights 2e-3 absolute);
3. invariance, bit for bit: alone, in slots 0, 2 and 4 of five, beside inactive neighbours, from a clone taken mid-loop;
4. the map staged into LDS and read in place from device memory: the same bits;
5. w_obs = 0 with a map set: the bits of a batch that never saw cost or map (the plain instance);
6. the dual loop: the fused period against its pieces bit for bit, `BatchDualSVMPC` beside three `DualSVMPC(fused=True)`;
7. plumbing: one launch per call, the refusal without a map before any launch, the refusals that stay, the example.
"""
import copy
import importlib.util
import os

import numpy as np
import pytest
import torch

import skid_nav_cases as cases
from helpers import elemerr
from test_gpu_svmpc_batch import TOL

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GETTERS = ("THETA", "PRIOR_MEANS", "PRIOR_MIX", "A_MAT", "COSTS", "SCORE", "PHI", "LOG_L", "LOG_P", "A_MIX", "ACTIONS")
UP2 = ("x_icr", "wheel_radius")
MPF_STEPS = 4


def _L():
    from dust_amd import _lib

    return _lib


def _records(b, forward=True):
    L = _L()
    return {n: b.get(getattr(L, "SVB_" + n)) for n in GETTERS if forward or n != "LOG_P"}


def _scenario(N, S, M, H, **kw):
    """a navigation scenario of these sizes: (x_icr, wheel_radius) sampled from the box of skid_nav_cases.XW, the 4 m x 4 m map at cells of
    0.1 m (50 words: staged into LDS), w_obs = 10"""
    return dict(cases.ROLLOUT_BY_TAG["fullcov"], N=N, S=S, M=M, H=H, a_cov=None, **kw)


def _proto_kw(s, **kw):
    """Context keywords of scenario s with its map"""
    return dict(cases.context_kwargs(s, **dict(dict(kernel="K1", lr=0.05), **kw)), grid=cases.make_map(s))


def _particles(rng, s, shape=()):
    """prior means round the scenario's forward command, particles round them"""
    N, H = s["N"], s["H"]
    mu = (s["fwd"] + 0.4 * rng.standard_normal(shape + (N, H, 2))).astype(np.float32)
    return mu, (mu + 0.3 * rng.standard_normal(shape + (N, H, 2))).astype(np.float32)


# ------------------------------------------------------------------------------------------------ 1. the reference's fixtures
FIXTURES = ["nominal", "ragged", "p3_log", "scalar", "offmap", "bigmap"]


@pytest.mark.parametrize("name", FIXTURES)
def test_fixtures_vs_reference_in_the_middle_slot(golden, name):
    """One optimize step of B = 3 from theta = a_mat0, the fixture's a_seq0, the recorded eps and the recorded dynamics samples in slot 1
    (the neighbours get other noise): the actions bit for bit, costs, the a_mat update and a_mix at the fixture's own tolerances (the
    nearer of the reference's fp32 and float64 values, as test_gpu_skid_nav.py), the costs >= 5 tolerances from every `_off` variant.
    `bigmap` (5000 words) reads the map in place, every other fixture from LDS."""
    from dust_amd import Context

    L = _L()
    s = cases.ROLLOUT_BY_TAG[name]
    g = golden(cases.fixture_name(s))
    c = Context(grid=cases.unpack_map(g), **cases.context_kwargs(s, kernel="K1", lr=0.05))
    c.set_theta(g["a_mat0"])
    c.set_prior(g["a_mat0"])
    c.set_a_mat(g["a_mat0"])
    c.set_a_seq(g["a_seq0"])
    rng = np.random.default_rng(1)

    def three(x, noise=False):
        x = np.asarray(x, np.float32)
        side = rng.standard_normal(x.shape).astype(np.float32) if noise else x
        return np.stack([side, x, side])

    b = c.svmpc_batch(3)
    c.close()
    b.optimize(np.stack([g["state"]] * 3), 1, eps=three(g["eps"][None], noise=True), params=three(g["params"][None]) if "params" in g else None,
               keep_actions=True)
    got = dict(costs=b.get(L.SVB_COSTS)[1], a_mat1=b.get(L.SVB_A_MAT)[1], a_mix=b.get(L.SVB_A_MIX)[1])
    actions = b.get(L.SVB_ACTIONS)
    side_costs = b.get(L.SVB_COSTS)[0]
    b.close()
    assert np.array_equal(actions[1], g["ext_actions"]), "theta + L eps must be bit-exact"
    assert not np.array_equal(actions[0], actions[1]) and not np.array_equal(side_costs, got["costs"])  # (the neighbours ran other noise)
    errs = {q: min(elemerr(v, g[q]), elemerr(v, cases.twin(g, q))) for q, v in got.items()}
    print(name + "  " + "  ".join("%s %.1e/%.1e" % (q, e, float(g["tol_" + q])) for q, e in errs.items()))
    for q, e in errs.items():
        assert e < float(g["tol_" + q]), (name, q, e, float(g["tol_" + q]))
    for v in s["offs"]:
        assert elemerr(g["costs_off_" + v], got["costs"]) >= 5 * float(g["tol_costs"]), (name, v)


# ------------------------------------------------------------------------------------------------ 2. against a lone context
SHAPES = [
    # N, S, M, H, options
    (8, 32, 3, 10, {}),                          # test_gpu_svmpc_batch.py's skid-steer shape (SGD, K1)
    (5, 7, 8, 15, dict(optimizer="Adam")),       # G = 8 dynamics groups in phase C; D = 30: the last Philox block of a row is partial
    (4, 16, 2, 6, dict(kernel="IMQ")),
]


@pytest.mark.parametrize("ext_noise", [True, False], ids=["recorded", "device"])
@pytest.mark.parametrize("N,S,M,H,opts", SHAPES)
def test_batch_equals_a_lone_context(N, S, M, H, opts, ext_noise):
    """test_gpu_svmpc_batch.py test_batch_equals_a_lone_context on the navigation family: three ticks (two iterations + forward) of a lone
    context and of environment 1 of a batch of two; after every tick the lone context takes over the batch's particles and a_mat."""
    from dust_amd import Context

    L = _L()
    s = _scenario(N, S, M, H)
    kw = _proto_kw(s, seed=77, **opts)
    st = np.array(s["state0"], np.float32)
    draw = lambda rng, n: rng.uniform(s["lo"], s["hi"], (n, M, 2)).astype(np.float32)
    rng = np.random.default_rng(5)
    mu, th = _particles(rng, s)
    lone = Context(**kw)
    lone.set_theta(th)
    lone.set_prior(mu)
    lone.set_a_mat(th)
    batch = lone.svmpc_batch(2, seeds=[5, kw["seed"]])  # environment 1 draws with the lone context's key
    iters = 2
    states = np.stack([st, st])
    worst = {}
    if not ext_noise:  # the first iteration's actions: the particles are equal by construction, so are the draws
        bc, lc = batch.clone(), lone.clone()
        p1 = draw(np.random.default_rng(9), 1)
        bc.optimize(states, 1, params=np.stack([p1, p1]), keep_actions=True)
        _, acts = lc.likelihood_sample(st, None, p1[0], want_actions=True)
        assert np.array_equal(bc.get(L.SVB_ACTIONS)[1], acts), "device-drawn actions must be bit-equal"
        bc.close()
        lc.close()
    for t in range(3):
        eps = rng.standard_normal((iters, S, N, H, 2)).astype(np.float32) if ext_noise else None
        params = draw(rng, iters)
        a_l, pw_l = lone.svmpc_tick(st, iters, eps=eps, params=params)
        a_b, pw_b = batch.tick(states, iters, eps=None if eps is None else np.stack([eps, eps]), params=np.stack([params, params]))
        ll, lp = lone.get_log_weights()
        got = {n: batch.get(getattr(L, "SVB_" + n)) for n in GETTERS if n != "ACTIONS"}
        pairs = dict(costs=(got["COSTS"][1], lone.get_costs()), score=(got["SCORE"][1], lone.get_score()), phi=(got["PHI"][1], lone.get_phi()),
                     theta=(got["THETA"][1], lone.get_theta()), a_mat=(got["A_MAT"][1], lone.get_a_mat()), log_l=(got["LOG_L"][1], ll),
                     log_p=(got["LOG_P"][1], lp), a_seq=(a_b[1], a_l))
        for k, (x, y) in pairs.items():
            worst[k] = max(worst.get(k, 0.0), elemerr(x, y))
        worst["p_weights"] = max(worst.get("p_weights", 0.0), float(np.abs(pw_b[1] - pw_l).max()))
        print("N %d S %d M %d H %d %s t %d: " % (N, S, M, H, "recorded" if ext_noise else "device", t) + "  ".join("%s %.1e" % kv for kv in worst.items()))
        for k, (x, y) in pairs.items():
            assert elemerr(x, y) < (TOL if k in ("costs", "log_p") else 25 * TOL), (t, k, elemerr(x, y))
        assert np.abs(pw_b[1] - pw_l).max() < 2e-3, t
        assert np.array_equal(got["THETA"][0], got["THETA"][1]) == ext_noise  # (slot 0 has another key: other draws)
        lone.set_theta(got["THETA"][1])  # (the prior means alias the particles: they follow)
        lone.set_a_mat(got["A_MAT"][1])
    # the term is there: the same inputs without the weight give other costs
    lone.set_obstacle_cost(0.0)
    eps = rng.standard_normal((S, N, H, 2)).astype(np.float32)
    p = draw(rng, 1)
    batch.optimize(states, 1, eps=np.stack([eps[None], eps[None]]), params=np.stack([p, p]))
    nav_costs = batch.get(L.SVB_COSTS)[1]
    plain = lone.likelihood_sample(st, eps, p[0])
    assert elemerr(nav_costs, plain) > 100 * TOL
    batch.close()
    lone.close()


# ------------------------------------------------------------------------------------------------ 3. invariance
INV = dict(N=4, S=24, M=3, H=8)
ITERS, TICKS = 2, 2


def _env_inputs(rng, s, iters=ITERS, ticks=TICKS):
    N, S, M, H = s["N"], s["S"], s["M"], s["H"]
    mu, th = _particles(rng, s)
    return dict(mu=mu, theta=th, a_mat=(s["fwd"] + 0.4 * rng.standard_normal((N, H, 2))).astype(np.float32),
                state=(np.array(s["state0"], np.float32) + 0.05 * rng.standard_normal(5)).astype(np.float32), seed=int(rng.integers(1, 1 << 40)),
                eps=rng.standard_normal((ticks, iters, S, N, H, 2)).astype(np.float32),
                params=rng.uniform(s["lo"], s["hi"], (ticks, iters, M, 2)).astype(np.float32))


def _fill(b, envs):
    L = _L()
    b.set(L.SVB_THETA, np.stack([e["theta"] for e in envs]))
    b.set(L.SVB_PRIOR_MEANS, np.stack([e["mu"] for e in envs]))
    b.set(L.SVB_A_MAT, np.stack([e["a_mat"] for e in envs]))


def _run_slots(proto, envs, active, ext_noise, iters=ITERS, ticks=TICKS, clone_after=None):
    """`envs`: one input set per slot -> per tick, the records and outputs of every slot (and the clone's, taken after tick `clone_after`)"""
    b = proto.svmpc_batch(len(envs), seeds=[e["seed"] for e in envs])
    _fill(b, envs)
    out, twin, out_twin = [], None, []
    for t in range(ticks):
        args = dict(eps=np.stack([e["eps"][t] for e in envs]) if ext_noise else None, params=np.stack([e["params"][t] for e in envs]),
                    active=active, keep_actions=True)
        states = np.stack([e["state"] for e in envs])
        a_seq, pw = b.tick(states, iters, **args)
        out.append(dict(_records(b), a_seq=a_seq, pw=pw))
        if twin is not None:
            a2, p2 = twin.tick(states, iters, **args)
            out_twin.append(dict(_records(twin), a_seq=a2, pw=p2))
        if clone_after == t:
            twin = b.clone()
    b.close()
    if twin is not None:
        twin.close()
    return out, out_twin


@pytest.mark.parametrize("ext_noise", [True, False], ids=["recorded", "device"])
def test_an_environment_does_not_depend_on_its_batch(ext_noise):
    """the method of test_gpu_svmpc_batch.py test_an_environment_does_not_depend_on_its_batch on a navigation prototype (Adam)"""
    from dust_amd import Context

    L = _L()
    s = _scenario(**INV)
    proto = Context(**_proto_kw(s, optimizer="Adam", seed=3))
    rng = np.random.default_rng(11)
    me = _env_inputs(rng, s)
    others = [_env_inputs(rng, s) for _ in range(4)]
    alone, _ = _run_slots(proto, [me], None, ext_noise)

    def same(rec, slot, ref):
        for t in range(len(ref)):
            for k, v in ref[t].items():
                assert np.array_equal(rec[t][k][slot], v[0]), (slot, t, k)

    for slot in (0, 2, 4):
        envs = others[:slot] + [me] + others[slot:]
        rec, twin = _run_slots(proto, envs, None, ext_noise, clone_after=0)
        same(rec, slot, alone)
        for k, v in rec[1].items():  # the clone taken after the first tick - it carries the map and the weight - continues identically
            assert np.array_equal(twin[0][k], v), k
    # the term is there: the same environment under a prototype without the weight computes other costs
    proto0 = Context(**dict(_proto_kw(s, optimizer="Adam", seed=3), w_obs=0.0))
    plain, _ = _run_slots(proto0, [me], None, ext_noise, ticks=1)
    proto0.close()
    assert elemerr(plain[0]["COSTS"], alone[0]["COSTS"]) > 100 * TOL
    # ... and beside inactive neighbours, whose rows stay untouched
    envs = others[:1] + [me] + others[1:]
    mask = np.array([0, 1, 0, 0, 0], np.uint8)
    b = proto.svmpc_batch(5, seeds=[e["seed"] for e in envs])
    _fill(b, envs)
    states = np.stack([e["state"] for e in envs])
    settable = (L.SVB_THETA, L.SVB_PRIOR_MEANS, L.SVB_PRIOR_MIX, L.SVB_A_MAT)
    keep = [b.get(w) for w in settable]
    for t in range(TICKS):
        a_seq, pw = b.tick(states, ITERS, eps=np.stack([e["eps"][t] for e in envs]) if ext_noise else None,
                           params=np.stack([e["params"][t] for e in envs]), active=mask, keep_actions=True)
        rec = dict(_records(b), a_seq=a_seq, pw=pw)
        for k, v in alone[t].items():
            assert np.array_equal(rec[k][1], v[0]), (t, k)
        assert np.isnan(a_seq[[0, 2, 3, 4]]).all() and np.isnan(pw[[0, 2, 3, 4]]).all()  # rows of inactive environments are not written
    for w, v in zip(settable, keep):
        assert np.array_equal(np.delete(b.get(w), 1, 0), np.delete(v, 1, 0))
    b.close()
    proto.close()


# ------------------------------------------------------------------------------------------------ 4. both map paths
@pytest.mark.parametrize("ext_noise", [True, False], ids=["recorded", "device"])
def test_both_map_paths_are_bit_identical(ext_noise, monkeypatch):
    """The same batch with the map staged into LDS (the default up to 4096 words) and read in place from device memory (the development
    switch DUST_NAV_GRID_HBM=1, read when a context is created - the prototype and the batch's own copy of it): every record and both
    outputs carry the same bits"""
    from dust_amd import Context

    s = _scenario(**INV)
    kw = _proto_kw(s, seed=3)
    rng = np.random.default_rng(12)
    envs = [_env_inputs(rng, s) for _ in range(3)]

    def run():
        proto = Context(**kw)
        b = proto.svmpc_batch(len(envs), seeds=[e["seed"] for e in envs])
        proto.close()
        _fill(b, envs)
        return b

    lds = run()
    monkeypatch.setenv("DUST_NAV_GRID_HBM", "1")
    hbm = run()
    monkeypatch.delenv("DUST_NAV_GRID_HBM")
    states = np.stack([e["state"] for e in envs])
    for t in range(TICKS):  # (the switch was read at creation: deleting it changes nothing for `hbm`)
        args = dict(eps=np.stack([e["eps"][t] for e in envs]) if ext_noise else None, params=np.stack([e["params"][t] for e in envs]), keep_actions=True)
        a1, p1 = lds.tick(states, ITERS, **args)
        a2, p2 = hbm.tick(states, ITERS, **args)
        assert np.array_equal(a1, a2) and np.array_equal(p1, p2), t
        r1, r2 = _records(lds), _records(hbm)
        for k in GETTERS:
            assert np.array_equal(r1[k], r2[k]), (t, k)
        assert np.isfinite(r1["THETA"]).all() and np.isfinite(r1["COSTS"]).all()
    lds.close()
    hbm.close()


# ------------------------------------------------------------------------------------------------ 5. w_obs = 0
@pytest.mark.parametrize("ext_noise", [True, False], ids=["recorded", "device"])
def test_w_obs_zero_with_a_grid_runs_the_plain_instance(ext_noise):
    """a prototype with a map and w_obs = 0 against one that never saw cost or map: every record and both outputs bit-equal"""
    from dust_amd import Context

    s = _scenario(**INV)
    rng = np.random.default_rng(13)
    envs = [_env_inputs(rng, s) for _ in range(2)]
    kw = cases.context_kwargs(s, kernel="K1", lr=0.05, seed=3)
    kw.pop("w_obs")
    plain = Context(**kw)
    zero = Context(**dict(_proto_kw(s, seed=3), w_obs=0.0))
    nav = Context(**_proto_kw(s, seed=3))
    a, _ = _run_slots(plain, envs, None, ext_noise)
    b, _ = _run_slots(zero, envs, None, ext_noise)
    c, _ = _run_slots(nav, envs, None, ext_noise, ticks=1)
    for o in (plain, zero, nav):
        o.close()
    for t in range(TICKS):
        for k, v in a[t].items():
            assert np.array_equal(b[t][k], v), (t, k)
    assert elemerr(c[0]["COSTS"], a[0]["COSTS"]) > 100 * TOL  # (with the weight: other costs)


# ------------------------------------------------------------------------------------------------ 6. the dual loop
@pytest.fixture
def single_workgroup_filters(monkeypatch):
    """lone filters run the single-workgroup kernel whose arithmetic the batch repeats (the switch is read in dust_mpf_create)"""
    monkeypatch.setenv("DUST_MPF_GRID", "0")


def _dual_setup(N, S, M, H, Mp, B, seeds, opt):
    """-> (navigation controller batch, skid-steer filter batch over (x_icr, wheel_radius), states [B, 5])"""
    from dust_amd import Context, MpfContext

    s = _scenario(N, S, M, H)
    c = Context(**_proto_kw(s, optimizer=opt, seed=77))
    sb = c.svmpc_batch(B, seeds=seeds)
    c.close()
    centre = np.array([cases.DEFAULTS[k] for k in UP2], np.float32)
    mus, ths, ams, xs, states = [], [], [], [], []
    for e in range(B):
        rng = np.random.default_rng(1000 + e)
        mu, th = _particles(rng, s)
        mus.append(mu)
        ths.append(th)
        ams.append((s["fwd"] + 0.4 * rng.standard_normal((N, H, 2))).astype(np.float32))
        xs.append((centre * (1.0 + 0.05 * rng.standard_normal((Mp, 2)))).astype(np.float32))
        states.append((np.array(s["state0"], np.float32) + 0.01 * rng.standard_normal(5)).astype(np.float32))
    _fill(sb, [dict(theta=t, mu=m, a_mat=a) for t, m, a in zip(ths, mus, ams)])
    m = MpfContext(xs[0], states[0], model="skid_steer", uncertain_params=UP2, obs_std=0.2, lr=1e-3 if opt == "Adam" else 1e-6, init_bw=0.01,
                   optimizer=opt, log_space=False, dt=s["dt"], min_a=s["bounds"][0], max_a=s["bounds"][1])
    mb = m.batch(B)
    m.close()
    mb.set_particles(np.stack(xs))
    states = np.stack(states)
    mb.set_obs(states)
    return sb, mb, states


def _plant(state, action):
    """a small host plant: any deterministic map does"""
    new = state.copy()
    new[: action.size] += np.float32(0.02) * np.tanh(action)
    new[-1] += np.float32(0.01)
    return new.astype(np.float32)


@pytest.mark.parametrize("device_noise", [False, True], ids=["recorded", "device"])
@pytest.mark.parametrize("Mp,M,opt,bw", [(3, 3, "Adam", 0.01), (48, 8, "SGD", None)], ids=["Mp3-M3", "Mp48-M8"])
def test_fused_period_equals_its_pieces(Mp, M, opt, bw, device_noise):
    """test_gpu_svmpc_dual_batch.py test_fused_period_equals_its_pieces on the navigation family (svmpc_skid_nav_prior_batch_kernel): three
    consecutive periods of B = 3 (the first without a filter update); before each, clones of both batches run the pieces -
    dust_mpf_batch_optimize, then dust_svmpc_batch_tick (svmpc_skid_nav_batch_kernel) fed params_out.  Bit for bit."""
    B, N, S, H, n_steps = 3, 4, 16, 6, 3
    sb, mb, states = _dual_setup(N, S, M, H, Mp, B, [7, 11, 5], opt)
    rng = np.random.default_rng(N + S + M)
    prev = None
    for t in range(3):
        sb2, mb2 = sb.clone(), mb.clone()
        eps = None if device_noise else rng.standard_normal((B, n_steps, S, N, H, 2)).astype(np.float32)
        keys = [100 + t + (b << 32) for b in range(B)]
        a1, pw1, rows, bwu = sb.dual_tick(mb, states, prev, n_steps=n_steps, eps=eps, mpf_steps=MPF_STEPS, mpf_bw=bw, seeds=keys, want_params=True,
                                          keep_actions=True)
        assert rows.shape == (B, n_steps, M, 2)
        if prev is None:
            assert (bwu == 0.0).all(), t
        else:
            _, bw2 = mb2.optimize(prev, states, bw, MPF_STEPS)
            assert np.array_equal(bwu, bw2), (t, bwu, bw2)
        a2, pw2 = sb2.tick(states, n_steps, eps=eps, params=rows, keep_actions=True)
        assert np.array_equal(mb.get_particles(), mb2.get_particles()) and np.array_equal(mb.get_prior_bw(), mb2.get_prior_bw()), t
        assert np.array_equal(a1, a2) and np.array_equal(pw1, pw2), t
        r1, r2 = _records(sb), _records(sb2)
        for k in GETTERS:
            assert np.array_equal(r1[k], r2[k]), (t, k)
        assert np.isfinite(a1).all() and np.isfinite(rows).all() and np.isfinite(r1["THETA"]).all() and np.isfinite(mb.get_particles()).all(), t
        if t == 0:  # the term is there: one more iteration from equal particles, with and without the weight, gives other costs
            sb0, mb0 = sb2.clone(), mb2.clone()
            sb0.ctx.set_obstacle_cost(0.0)
            sb0.dual_tick(mb0, states, prev, n_steps=1, eps=None if eps is None else eps[:, :1], mpf_steps=MPF_STEPS, mpf_bw=bw, seeds=keys)
            sb2.dual_tick(mb2, states, prev, n_steps=1, eps=None if eps is None else eps[:, :1], mpf_steps=MPF_STEPS, mpf_bw=bw, seeds=keys)
            L = _L()
            assert elemerr(sb0.get(L.SVB_COSTS), sb2.get(L.SVB_COSTS)) > 100 * TOL
            sb0.close()
            mb0.close()
        sb2.close()
        mb2.close()
        prev = a1[:, 0].copy()
        states = np.stack([_plant(states[b], prev[b]) for b in range(B)])
    sb.close()
    mb.close()


def _nav_cost(s, grid, w_ctrl):
    from dust_amd.costs import NavigationCost
    from dust_amd.utils.obstacle_map import ObstacleMap

    om = ObstacleMap(list(s["map_dim"]), s["cell"])
    om.map = np.asarray(grid, np.float64)
    return NavigationCost(cases.GOAL, cases.W_STATE, cases.W_TERM, torch.tensor(w_ctrl), obst_map=om, w_obs=s["w_obs"])


def _mirror(B, seed):
    """-> (BatchDualSVMPC of B environments, [DualSVMPC(fused=True, seed=seed + (b << 32))] over the same configuration, states [B, 5]):
    SkidSteerRobot with all three parameters uncertain in log space under a NavigationCost (the configuration of test_gpu_skid_nav.py
    test_dual_svmpc_with_the_navigation_cost_fused_equals_unfused)"""
    from dust_amd.controllers import BatchDualSVMPC, DualSVMPC, MultiDISCO
    from dust_amd.inference import MPF, SVMPC, BatchSVMPC, ExponentiatedUtility, GaussianLikelihood, get_gmm
    from dust_amd.kernels import RBFKernel
    from dust_amd.models import SkidSteerRobot
    from mpf_skid_cases import NAMES3, particles

    N, S, M, H, Mp = 4, 16, 3, 6, 48
    s = cases.ROLLOUT_BY_TAG["nominal"]
    cost = _nav_cost(s, cases.make_map(s), (0.1, 0.1))
    rng = np.random.default_rng(21)
    mu = torch.tensor((0.3 + 0.2 * rng.standard_normal((N, H, 2))).astype(np.float32))
    th = mu + torch.tensor((0.1 * rng.standard_normal((N, H, 2))).astype(np.float32))
    x0 = torch.tensor(np.stack([particles(NAMES3, Mp, True, 78 + b, 0.2) for b in range(B)]))
    states = torch.tensor(s["state0"])[None] + torch.tensor((0.01 * rng.standard_normal((B, 5))).astype(np.float32))
    cov = 0.09 * torch.eye(2)

    def parts(b):
        model = SkidSteerRobot(delta_t=0.1, uncertain_params=NAMES3)
        ctrl = MultiDISCO(observation_space=model.observation_space, action_space=model.action_space, hz_len=H, action_samples=S, params_samples=M,
                          temperature=2.0, a_cov=cov, inst_cost_fn=cost.inst_cost, term_cost_fn=cost.term_cost, params_sampling=True, n_policies=N,
                          params_log_space=True, seed=40 + b)
        ctrl.a_mat = th.clone()
        ctrl.return_rollouts = False
        mpf = MPF(init_particles=x0[b].clone(), likelihood=GaussianLikelihood(initial_obs=states[b], obs_std=0.05, model=model, log_space=True),
                  optimizer_class=torch.optim.SGD, lr=1e-4, bw=0.3, bw_scale=1.0)
        kw = dict(init_particles=th.clone(), prior=get_gmm(mu, torch.ones(N), cov), kernel=RBFKernel(), n_particles=N, n_steps=2,
                  likelihood=ExponentiatedUtility(alpha=0.5, n_samples=S, controller=ctrl, model=model), optimizer_class=torch.optim.SGD, lr=0.05)
        return kw, mpf

    lones = []
    for b in range(B):
        kw, mpf = parts(b)
        lones.append(DualSVMPC(SVMPC(**kw), mpf, mpf_bw=0.3, mpf_steps=MPF_STEPS, fused=True, seed=seed + (b << 32)))
    kw, mpf = parts(0)
    loop = BatchDualSVMPC(BatchSVMPC(B, seeds=[40 + b for b in range(B)], **kw), mpf, mpf_bw=0.3, mpf_steps=MPF_STEPS, seed=seed, init_particles=x0)
    return loop, lones, states


def test_class_against_lone_objects(single_workgroup_filters):
    """test_gpu_svmpc_dual_batch.py test_class_against_lone_objects with a NavigationCost: BatchDualSVMPC (B = 3) and three
    DualSVMPC(fused=True, seed=seed + (b << 32)) under one prescribed, open-loop sequence of states and previous actions over three
    periods, device-drawn noise under equal keys.  Filters (48 particles: the single-workgroup kernel): particles bit for bit, every
    period.  Controllers: first-divergence form at the tolerances of item 2 (a_seq and theta 25 TOL element-wise, p_weights 2e-3
    absolute).  A deep copy of the class taken after the first period continues bit-equal."""
    B, seed = 3, 20260
    loop, lones, states = _mirror(B, seed)
    twin = None
    rng = np.random.default_rng(4)
    for t in range(3):
        if t > 0:
            actions = torch.from_numpy((0.3 * rng.standard_normal((B, 2))).astype(np.float32))
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
            ea, ep = elemerr(a_b[b].numpy(), outs[b][0].numpy()), float((pw_b[b] - outs[b][1]).abs().max())
            et = elemerr(loop.theta[b].numpy(), lo.theta.numpy())
            print("t %d b %d: a_seq %.1e  p_weights %.1e  theta %.1e" % (t, b, ea, ep, et))
            assert ea < 25 * TOL and ep < 2e-3 and et < 25 * TOL, (t, b, ea, ep, et)
        for b, lo in enumerate(lones):  # first-divergence form: the lone objects take the batch's particles over
            lo.svmpc.theta = loop.theta[b]
        if t == 0:
            twin = copy.deepcopy(loop)
    inner = loop.svmpc._batch.ctx
    assert float(inner.cfg.cell_size) == pytest.approx(cases.ROLLOUT_BY_TAG["nominal"]["cell"]) and loop.ticks == 3


# ------------------------------------------------------------------------------------------------ 7. plumbing
def test_one_launch_per_call_and_the_refusal_without_a_map():
    from dust_amd import Context

    L = _L()
    s = _scenario(**INV)
    B = 3
    rng = np.random.default_rng(14)
    envs = [_env_inputs(rng, s) for _ in range(B)]
    states = np.stack([e["state"] for e in envs])
    params = np.stack([e["params"][0] for e in envs])
    c = Context(**_proto_kw(s, seed=1))
    b = c.svmpc_batch(B)
    c.close()
    _fill(b, envs)
    b.ctx.profile(True)
    count = lambda o: o.ctx.profile_get().get("svmpc_batch_kernel", (0.0, 0))[1]
    total = lambda o: sum(v[1] for v in o.ctx.profile_get().values())
    b.optimize(states, ITERS, params=params)
    assert count(b) == 1 == total(b)
    b.forward()
    assert count(b) == 2 == total(b)
    b.tick(states, ITERS, params=params)
    assert count(b) == 3 == total(b)
    b.tick(states, ITERS, params=params, active=np.arange(B) % 2 == 0, want_outputs=False)
    assert count(b) == 4 == total(b)
    b.close()
    # a prototype with the weight and no map: DUST_ERR_STATE from dust_svmpc_batch_create, nothing launched, the prototype as it was
    kw = _proto_kw(s, seed=1)
    kw.pop("grid")
    p = Context(**kw)
    p.set_theta(envs[0]["theta"])
    p.set_a_mat(envs[0]["a_mat"])
    p.profile(True)
    with pytest.raises(L.DustError, match="no occupancy grid was supplied") as e:
        p.svmpc_batch(2)
    assert e.value.status == L.ERR_STATE and p.profile_get() == {}
    assert np.array_equal(p.get_theta(), envs[0]["theta"]) and np.array_equal(p.get_a_mat(), envs[0]["a_mat"])
    p.set_grid(cases.make_map(s))  # ... and with the map it is accepted
    p.svmpc_batch(2).close()
    p.close()
    # a live batch whose weight is switched on without a map: every call answers DUST_ERR_STATE before any launch, every getter unchanged
    kw.pop("w_obs")
    p = Context(**kw)
    b = p.svmpc_batch(B)
    p.close()
    _fill(b, envs)
    b.tick(states, ITERS, params=params, keep_actions=True)
    before = _records(b)
    b.ctx.profile(True)
    b.ctx.set_obstacle_cost(s["w_obs"])
    for call in (lambda: b.optimize(states, 1, params=params[:, :1]), lambda: b.tick(states, ITERS, params=params), lambda: b.forward()):
        with pytest.raises(L.DustError, match="no occupancy grid was supplied") as e:
            call()
        assert e.value.status == L.ERR_STATE
    assert total(b) == 0
    now = _records(b)
    for k, v in before.items():
        assert np.array_equal(now[k], v), k
    b.ctx.set_obstacle_cost(0.0)
    b.tick(states, ITERS, params=params)
    assert count(b) == 1 == total(b)
    b.close()


def test_the_refusals_that_stay(golden):
    """sigma-point weights, a full a_cov and ctrl_penalty != 1 on a navigation prototype: DUST_ERR_UNSUPPORTED from dust_svmpc_batch_create"""
    from dust_amd import Context

    L = _L()
    s = _scenario(**INV)
    u = cases.ROLLOUT_BY_TAG["ut_p1"]
    gu = golden(cases.fixture_name(u))
    sigma = Context(grid=cases.unpack_map(gu), **cases.context_kwargs(u, kernel="K1", lr=0.05))
    sigma.set_param_weights(gu["loc_weights"])
    full = Context(**_proto_kw(dict(s, a_cov=cases.FULL_COV)))
    areg = Context(**_proto_kw(dict(s, ctrl_penalty=cases.CTRL_PENALTY)))
    for c, what in ((sigma, "sigma-point"), (full, "diagonal covariances"), (areg, "ctrl_penalty = 1")):
        with pytest.raises(L.DustError, match=what) as e:
            c.svmpc_batch(2)
        assert e.value.status == L.ERR_UNSUPPORTED, what
        c.close()


def test_example_runs_three_periods():
    path = os.path.join(ROOT, "examples", "skid_steer_batch_example.py")
    spec = importlib.util.spec_from_file_location("skid_steer_batch_example", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    track = mod.main(["--tiny"])
    B, ticks = mod.TINY["envs"], mod.TINY["ticks"]
    assert ticks == 3 and tuple(track.shape) == (ticks + 1, B, 5) and bool(torch.isfinite(track).all())
    assert all(not torch.equal(track[0, b], track[-1, b]) for b in range(B))
    assert len({tuple(track[-1, b].tolist()) for b in range(B)}) == B
