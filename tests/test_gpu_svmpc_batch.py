"""SVMPC over a batch of plants (dust_amd/csrc/svmpc_batch.hpp, dust_svmpc_batch_*, `BatchSVMPC`): B independent ticks in ONE launch.

1. invariance, bit for bit: an environment computes the same alone, in any slot of a batch, beside inactive neighbours, from a clone;
2. against a lone context on the same inputs, first-divergence form (tests/test_gpu_tick2.py test_tick2_equals_launch_per_iteration and
   its tolerances: costs 2e-5 element-wise, what lies downstream of exp(-alpha cost) 5e-4, p_weights 2e-3 absolute);
3. the reference, through the cart-pole tick fixtures (the stages and the stored tolerances of tests/test_gpu_cartpole.py);
4. one whole tick against the CPU oracle (tests/test_gpu_tick2.py test_tick2_against_oracle_whole_tick's 2e-3);
5. plumbing: one launch per call, refusals before any launch, `BatchSVMPC` against B `SVMPC` objects, the example.
"""
import copy
import importlib.util
import os

import numpy as np
import pytest
import torch

from helpers import elemerr, relerr

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = 2e-5


def _L():
    from dust_amd import _lib

    return _lib


def _records(b, forward=True, actions=False):
    L = _L()
    names = ["THETA", "PRIOR_MEANS", "PRIOR_MIX", "A_MAT", "COSTS", "SCORE", "PHI", "LOG_L", "A_MIX"] + (["LOG_P"] if forward else []) + \
        (["ACTIONS"] if actions else [])
    return {n: b.get(getattr(L, "SVB_" + n)) for n in names}


# ------------------------------------------------------------------------------------------------ the shapes of item 2
def _family(model, N, S, M, H, opts, seed=77):
    """-> (Context keywords, state, a draw of [n, M, P] dynamics samples or None, scale of the particles)"""
    kw = dict(kernel=opts.get("kernel", "K1"), optimizer=opts.get("optimizer", "SGD"), weighted_prior=opts.get("weighted_prior", False),
              roll_strategy=opts.get("roll", "repeat"), seed=seed)
    if "lik" in opts:
        kw["likelihood"] = opts["lik"]
    if model == "pendulum":
        kw.update(model=model, N=N, S=S, M=M, H=H, lr=2.0, sigma_a=2.0, sigma_p=2.0)
        if M > 1:
            kw["uncertain_params"] = ("length", "mass")
        return kw, np.array([3.0, 0.0], np.float32), (lambda rng, n: (1.0 + 0.1 * rng.standard_normal((n, M, 2))).astype(np.float32)) if M > 1 else None, 1.0
    if model == "particle":
        from oracle import grid_4x4_map

        kw.update(model=model, N=N, S=S, M=M, H=H, lr=100.0, sigma_a=5.0, sigma_p=5.0, grid=grid_4x4_map())
        if M > 1:
            kw["uncertain_params"] = ("mass",)
        return kw, np.array([-9.0, -9.0, 0.0, 0.0], np.float32), (lambda rng, n: (1.0 + 0.1 * rng.standard_normal((n, M, 1))).astype(np.float32)) if M > 1 else None, 1.0
    if model == "skid_steer":
        import skid_cases as sc

        s = sc.R("batch", N, S, H, M, ("x_icr", "wheel_radius"), "uniform", None, 0, **sc.XW)
        kw = sc.controller_kwargs(s, lr=0.05, **kw)
        lo, hi = np.asarray(sc.XW["lo"]), np.asarray(sc.XW["hi"])
        return kw, np.asarray(sc.STATE0, np.float32), lambda rng, n: rng.uniform(lo, hi, (n, M, 2)).astype(np.float32), 0.3
    import cartpole_cases as cc

    s = cc.ROLLOUT_BY_TAG["params_log"]  # log-space parameters (length, f_mag, g, mu_p)
    s = dict(s, N=N, S=S, H=H, M=M)
    kw = cc.controller_kwargs(s, lr=0.05, **kw)
    loc, scale = np.asarray(s["loc"]), np.asarray(s["scale"])
    return kw, np.asarray(cc.STATE0, np.float32), lambda rng, n: (loc + scale * rng.standard_normal((n, M, 4))).astype(np.float32), 0.5


SHAPES = [
    # model, N, S, M, H, options
    ("pendulum", 3, 128, 8, 30, {}),                                         # the demo (SGD)
    ("pendulum", 1, 1, 1, 1, {}),
    ("pendulum", 33, 65, 1, 15, dict(optimizer="Adam")),
    ("pendulum", 64, 16, 1, 30, dict(kernel="IMQ", weighted_prior=True)),
    ("pendulum", 8, 63, 3, 12, dict(roll="mean", lik="ExpectedCost")),
    ("particle", 4, 64, 4, 40, {}),                                          # the 4 x 4 map, D = 80
    ("particle", 2, 16, 1, 64, {}),                                          # D = 128, the cap
    ("skid_steer", 8, 32, 3, 10, {}),
    ("cartpole", 8, 16, 3, 12, {}),                                          # log-space parameters
]
_measured = {}


@pytest.mark.parametrize("ext_noise", [True, False])
@pytest.mark.parametrize("model,N,S,M,H,opts", SHAPES)
def test_batch_equals_a_lone_context(model, N, S, M, H, opts, ext_noise):
    """Three ticks (two iterations + forward) of a lone context and of environment 1 of a batch of two, side by side; after every tick
    the lone context takes over the batch's particles, prior and a_mat, so every tick is a first-divergence comparison."""
    from dust_amd import Context

    L = _L()
    kw, st, draw, scale = _family(model, N, S, M, H, opts)
    da = 1 if model in ("pendulum", "cartpole") else 2
    rng = np.random.default_rng(5)
    mu = (scale * rng.standard_normal((N, H, da))).astype(np.float32)
    th = (mu + 2 * scale * rng.standard_normal((N, H, da))).astype(np.float32)
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
        p1 = None if draw is None else draw(np.random.default_rng(9), 1)
        bc.optimize(states, 1, params=None if p1 is None else np.stack([p1, p1]), keep_actions=True)
        _, acts = lc.likelihood_sample(st, None, None if p1 is None else p1[0], want_actions=True)
        assert np.array_equal(bc.get(L.SVB_ACTIONS)[1], acts), "device-drawn actions must be bit-equal"
        bc.close()
        lc.close()
    for t in range(3):
        eps = rng.standard_normal((iters, S, N, H, da)).astype(np.float32) if ext_noise else None
        params = None if draw is None else draw(rng, iters)
        a_l, pw_l = lone.svmpc_tick(st, iters, eps=eps, params=params)
        a_b, pw_b = batch.tick(states, iters, eps=None if eps is None else np.stack([eps, eps]),
                               params=None if params is None else np.stack([params, params]))
        ll, lp = lone.get_log_weights()
        got = _records(batch)
        pairs = dict(costs=(got["COSTS"][1], lone.get_costs()), score=(got["SCORE"][1], lone.get_score()), phi=(got["PHI"][1], lone.get_phi()),
                     theta=(got["THETA"][1], lone.get_theta()), a_mat=(got["A_MAT"][1], lone.get_a_mat()), log_l=(got["LOG_L"][1], ll),
                     log_p=(got["LOG_P"][1], lp), a_seq=(a_b[1], a_l))
        for k, (x, y) in pairs.items():
            e = elemerr(x, y)
            worst[k] = max(worst.get(k, 0.0), e)
            assert e < (TOL if k in ("costs", "log_p") else 25 * TOL), (t, k, e)  # (test_tick2_equals_launch_per_iteration holds log_p to TOL too)
        worst["p_weights"] = max(worst.get("p_weights", 0.0), float(np.abs(pw_b[1] - pw_l).max()))
        assert np.abs(pw_b[1] - pw_l).max() < 2e-3, t
        assert np.array_equal(got["THETA"][0], got["THETA"][1]) == ext_noise or N * H == 1  # (slot 0 has another key: other draws)
        lone.set_theta(got["THETA"][1])  # (the prior means alias the particles: they follow)
        lone.set_a_mat(got["A_MAT"][1])
        if opts.get("weighted_prior"):
            lone.svmpc_update_prior(pw_b[1])
    _measured[(model, N, S, M, H, ext_noise)] = worst
    print("%s N %d S %d M %d H %d %s: " % (model, N, S, M, H, "recorded" if ext_noise else "device") +
          "  ".join("%s %.1e" % kv for kv in worst.items()))
    batch.close()
    lone.close()


# ------------------------------------------------------------------------------------------------ 1. invariance
def _env_inputs(rng, N, S, M, H, iters, ticks):
    mu = rng.standard_normal((N, H, 1)).astype(np.float32)
    return dict(mu=mu, theta=(mu + 2 * rng.standard_normal((N, H, 1))).astype(np.float32), a_mat=rng.standard_normal((N, H, 1)).astype(np.float32),
                state=np.array([3.0 + 0.2 * rng.standard_normal(), 0.1 * rng.standard_normal()], np.float32), seed=int(rng.integers(1, 1 << 40)),
                eps=rng.standard_normal((ticks, iters, S, N, H, 1)).astype(np.float32),
                params=(1.0 + 0.1 * rng.standard_normal((ticks, iters, M, 2))).astype(np.float32))


def _run_slots(proto, envs, active, ext_noise, iters, ticks, clone_after=None):
    """`envs`: one input set per slot -> per tick, the records of every slot (and the clone's, taken after tick `clone_after`)"""
    L = _L()
    B = len(envs)
    b = proto.svmpc_batch(B, seeds=[e["seed"] for e in envs])
    b.set(L.SVB_THETA, np.stack([e["theta"] for e in envs]))
    b.set(L.SVB_PRIOR_MEANS, np.stack([e["mu"] for e in envs]))
    b.set(L.SVB_A_MAT, np.stack([e["a_mat"] for e in envs]))
    out, twin, out_twin = [], None, []
    for t in range(ticks):
        args = dict(eps=np.stack([e["eps"][t] for e in envs]) if ext_noise else None, params=np.stack([e["params"][t] for e in envs]),
                    active=active, keep_actions=True)
        states = np.stack([e["state"] for e in envs])
        a_seq, pw = b.tick(states, iters, **args)
        out.append(dict(_records(b, actions=True), a_seq=a_seq, pw=pw))
        if twin is not None:
            a2, p2 = twin.tick(states, iters, **args)
            out_twin.append(dict(_records(twin, actions=True), a_seq=a2, pw=p2))
        if clone_after == t:
            twin = b.clone()
    b.close()
    if twin is not None:
        twin.close()
    return out, out_twin


@pytest.mark.parametrize("ext_noise", [True, False])
def test_an_environment_does_not_depend_on_its_batch(ext_noise):
    from dust_amd import Context

    N, S, M, H, iters, ticks = 3, 128, 8, 30, 2, 2
    proto = Context(model="pendulum", N=N, S=S, M=M, H=H, kernel="K1", lr=2.0, sigma_a=2.0, sigma_p=2.0, optimizer="Adam",
                    uncertain_params=("length", "mass"), seed=3)
    rng = np.random.default_rng(11)
    me = _env_inputs(rng, N, S, M, H, iters, ticks)
    others = [_env_inputs(rng, N, S, M, H, iters, ticks) for _ in range(4)]
    alone, _ = _run_slots(proto, [me], None, ext_noise, iters, ticks)

    def same(rec, slot, ref):
        for t in range(ticks):
            for k, v in ref[t].items():
                assert np.array_equal(rec[t][k][slot], v[0]), (slot, t, k)

    for slot in (0, 1, 4):
        envs = others[:slot] + [me] + others[slot:]
        rec, twin = _run_slots(proto, envs, None, ext_noise, iters, ticks, clone_after=0)
        same(rec, slot, alone)
        for k, v in rec[1].items():  # the clone taken after the first tick continues identically, every slot
            assert np.array_equal(twin[0][k], v), k
    # ... and beside inactive neighbours, which keep everything
    L = _L()
    envs = others[:1] + [me] + others[1:]
    mask = np.array([0, 1, 0, 0, 0], np.uint8)
    b = proto.svmpc_batch(5, seeds=[e["seed"] for e in envs])
    b.set(L.SVB_THETA, np.stack([e["theta"] for e in envs]))
    b.set(L.SVB_PRIOR_MEANS, np.stack([e["mu"] for e in envs]))
    b.set(L.SVB_A_MAT, np.stack([e["a_mat"] for e in envs]))
    states = np.stack([e["state"] for e in envs])
    keep = [b.get(w) for w in (L.SVB_THETA, L.SVB_PRIOR_MEANS, L.SVB_PRIOR_MIX, L.SVB_A_MAT)]
    for t in range(ticks):
        a_seq, pw = b.tick(states, iters, eps=np.stack([e["eps"][t] for e in envs]) if ext_noise else None,
                           params=np.stack([e["params"][t] for e in envs]), active=mask, keep_actions=True)
        rec = dict(_records(b, actions=True), a_seq=a_seq, pw=pw)
        for k, v in alone[t].items():
            assert np.array_equal(rec[k][1], v[0]), (t, k)
        assert np.isnan(a_seq[[0, 2, 3, 4]]).all() and np.isnan(pw[[0, 2, 3, 4]]).all()  # rows of inactive environments are not written
    for w, v in zip((L.SVB_THETA, L.SVB_PRIOR_MEANS, L.SVB_PRIOR_MIX, L.SVB_A_MAT), keep):
        assert np.array_equal(np.delete(b.get(w), 1, 0), np.delete(v, 1, 0))
    # optimiser state and stream position of a sleeper are untouched: woken up alone, it computes its first tick
    first, _ = _run_slots(proto, [others[0]], None, ext_noise, iters, 1)
    a_seq, pw = b.tick(states, iters, eps=np.stack([e["eps"][0] for e in envs]) if ext_noise else None,
                       params=np.stack([e["params"][0] for e in envs]), active=np.array([1, 0, 0, 0, 0], np.uint8), keep_actions=True)
    rec = dict(_records(b, actions=True), a_seq=a_seq, pw=pw)
    for k, v in first[0].items():
        assert np.array_equal(rec[k][0], v[0]), k
    b.close()
    proto.close()


# ------------------------------------------------------------------------------------------------ 3. the reference's fixtures
@pytest.mark.parametrize("name", ["tick_k1_sgd", "tick_k1_adam"])
def test_cartpole_ticks_vs_reference_in_the_middle_slot(golden, name):
    """test_gpu_cartpole.py test_ticks_vs_reference's stages that run rollouts, in slot 1 of B = 3 (the neighbours get other noise)."""
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

    errs = {}
    b = c.svmpc_batch(3)
    for k in range(K):  # the updated particles: K optimiser steps from the recorded draws (Adam's state carried from step to step)
        b.optimize(states, 1, eps=three(g["eps"][k][None], noise=True), params=three(g["params"][k][None]))
        for q, v in (("costs", b.get(L.SVB_COSTS)[1]), ("theta_after", b.get(L.SVB_THETA)[1])):
            errs["%s[%d]" % (q, k)] = (min(elemerr(v, g[q][k]), elemerr(v, g[q + "_f64"][k])), float(g["tol_" + q]))
    assert elemerr(g["costs_off"], g["costs"][-1]) >= 10 * float(g["tol_costs"])
    assert elemerr(g["costs_off"], b.get(L.SVB_COSTS)[1]) >= 9 * float(g["tol_costs"])
    b.close()
    b = c.svmpc_batch(3)  # forward(): the state the reference was in before it - its particles, prior, last costs
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
    b.close()
    c.close()
    print(name + " " + "  ".join("%s %.1e/%.1e" % (q, e, t) for q, (e, t) in errs.items()))
    for q, (e, t) in errs.items():
        assert e < t, (name, q, e, t)


# ------------------------------------------------------------------------------------------------ 4. the oracle
def test_whole_tick_against_the_oracle():
    """BASELINE config 1's shape (pendulum, N 32, S 128, H 15, M 1), one tick of 3 iterations + forward in slot 1 of B = 2 against
    Oracle.tick_k1 fed the same noise (the bound of test_tick2_against_oracle_whole_tick)."""
    from dust_amd import Context
    from oracle import Oracle

    L = _L()
    N, S, H, K = 32, 128, 15, 3
    rng = np.random.default_rng(0)
    mu = rng.standard_normal((N, H, 1)).astype(np.float32)
    th = (mu + 2 * rng.standard_normal((N, H, 1))).astype(np.float32)
    c = Context(model="pendulum", N=N, S=S, M=1, H=H, kernel="K1", lr=2.0, sigma_a=2.0, sigma_p=2.0, seed=77)
    c.set_theta(th)
    c.set_prior(mu)
    c.set_a_mat(th)
    b = c.svmpc_batch(2)
    st = np.array([3.0, 0.0], np.float32)
    states = np.stack([st, st])
    eps0 = rng.standard_normal((2, 1, S, N, H, 1)).astype(np.float32)
    b.tick(states, 1, eps=eps0)  # afterwards the prior means alias the particles
    th1, mix, am = b.get(L.SVB_THETA)[1], b.get(L.SVB_PRIOR_MIX)[1], b.get(L.SVB_A_MAT)[1]
    eps = rng.standard_normal((2, K, S, N, H, 1)).astype(np.float32)
    a_seq, pw = b.tick(states, K, eps=eps)
    o = Oracle(model="pendulum", N=N, S=S, M=1, H=H)
    r = o.tick_k1(st, th1, th1, mix, 2.0, 2.0, eps[1], K, 1.0, 2.0, am)
    e = elemerr(b.get(L.SVB_THETA)[1], r["theta"])
    print("oracle: theta %.1e  p_weights %.1e" % (e, np.abs(pw[1] - r["p_weights"]).max()))
    assert e < 2e-3, e
    assert np.abs(pw[1] - r["p_weights"]).max() < 2e-3
    if np.sort(r["p_weights"])[-1] - np.sort(r["p_weights"])[-2] > 1e-2:
        assert elemerr(a_seq[1].reshape(-1), r["a_seq"].reshape(-1)) < 2e-3
    b.close()
    c.close()


# ------------------------------------------------------------------------------------------------ 5. plumbing
@pytest.mark.parametrize("B", [1, 5])
def test_one_launch_per_call_and_refusals_before_any_launch(B):
    from dust_amd import Context

    L = _L()
    N, S, H = 4, 32, 8
    c = Context(model="pendulum", N=N, S=S, M=1, H=H, kernel="K1", lr=1.0, sigma_a=2.0, sigma_p=2.0, seed=1)
    b = c.svmpc_batch(B)
    b.ctx.profile(True)
    states = np.tile(np.array([3.0, 0.0], np.float32), (B, 1))
    count = lambda: b.ctx.profile_get().get("svmpc_batch_kernel", (0.0, 0))[1]
    total = lambda: sum(v[1] for v in b.ctx.profile_get().values())
    with pytest.raises(L.DustError) as e:  # before any step has produced costs
        b.forward()
    assert e.value.status == L.ERR_STATE and total() == 0
    for what in (L.SVB_COSTS, L.SVB_LOG_P, L.SVB_ACTIONS):
        with pytest.raises(L.DustError) as e:
            b.get(what)
        assert e.value.status == L.ERR_STATE
    b.optimize(states, 3)
    assert count() == 1 == total()
    b.forward()
    assert count() == 2 == total()
    b.tick(states, 2)
    assert count() == 3 == total()
    b.tick(states, 1, active=np.arange(B) % 2 == 0, want_outputs=False)
    assert count() == 4 == total()
    lib, FP = L.load(), L.FP
    st = states.ctypes.data_as(FP)
    bad = np.zeros((B, 1, 1, 1), np.float32).ctypes.data_as(FP)
    refused = [
        (lib.dust_svmpc_batch_optimize(b._h, st, 1, None, None, L.STORE_STATES, None), L.ERR_UNSUPPORTED),
        (lib.dust_svmpc_batch_optimize(b._h, st, 1, None, None, L.EPS_F16, None), L.ERR_UNSUPPORTED),
        (lib.dust_svmpc_batch_optimize(b._h, st, 1, None, None, L.STORE_F16, None), L.ERR_UNSUPPORTED),
        (lib.dust_svmpc_batch_optimize(b._h, st, 1, None, bad, 0, None), L.ERR_INVALID),   # rows without uncertain parameters
        (lib.dust_svmpc_batch_optimize(b._h, None, 1, None, None, 0, None), L.ERR_INVALID),
        (lib.dust_svmpc_batch_optimize(b._h, st, -1, None, None, 0, None), L.ERR_INVALID),
        (lib.dust_svmpc_batch_tick(b._h, st, 0, None, None, 0, None, None, None), L.ERR_INVALID),
        (lib.dust_svmpc_batch_get(b._h, 11, bad), L.ERR_INVALID),
        (lib.dust_svmpc_batch_set(b._h, L.SVB_COSTS, bad), L.ERR_INVALID),
    ]
    for got, want in refused:
        assert got == want, (got, want)
    assert count() == 4 == total()
    b.close()
    c.close()
    # what dust_svmpc_batch_create refuses of a prototype, and of n_env
    for kw, status in ((dict(kernel="K2"), L.ERR_UNSUPPORTED), (dict(N=65), L.ERR_UNSUPPORTED), (dict(ctrl_penalty=0.6), L.ERR_UNSUPPORTED),
                       (dict(roll_strategy="resample"), L.ERR_UNSUPPORTED), (dict(S=1025), L.ERR_UNSUPPORTED)):
        p = Context(**dict(dict(model="pendulum", N=N, S=S, M=1, H=H, kernel="K1", lr=1.0, sigma_a=2.0, sigma_p=2.0), **kw))
        with pytest.raises(L.DustError) as e:
            p.svmpc_batch(2)
        assert e.value.status == status, kw
        p.close()
    p = Context(model="pendulum", N=N, S=S, M=1, H=H, kernel="K1", lr=1.0, sigma_a=2.0, sigma_p=2.0)
    for n in (0, 65536):
        with pytest.raises(L.DustError) as e:
            p.svmpc_batch(n)
        assert e.value.status == L.ERR_INVALID
    p.close()


def _mirror(cls, n_envs=None, seed=0, N=4, S=32, H=8, M=3):
    from dust_amd.controllers import MultiDISCO
    from dust_amd.costs import PendulumQuadCos
    from dust_amd.inference import ExponentiatedUtility, get_gmm
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
    kw = dict(init_particles=th, prior=prior, likelihood=lik, kernel=RBFKernel(), n_particles=N, n_steps=2, optimizer_class=torch.optim.Adam, lr=0.1)
    return cls(n_envs, **kw) if n_envs else cls(**kw)


def test_batch_svmpc_agrees_with_B_svmpc_objects():
    """three periods, recorded noise, the class's own parameter draws (one torch stream: the B objects draw in environment order, as the
    batch does), a deep copy of everything after the first period; tolerances of item 2"""
    import torch.distributions as dist

    from dust_amd.inference import SVMPC, BatchSVMPC

    B, N, S, H = 3, 4, 32, 8
    pd = dist.Independent(dist.Uniform(torch.tensor([0.8, 0.8]), torch.tensor([1.2, 1.2])), 1)
    batch = _mirror(BatchSVMPC, B)
    lone = [_mirror(SVMPC) for _ in range(B)]
    states = torch.tensor([[3.0, 0.0], [2.5, 0.2], [3.4, -0.1]])
    rng = np.random.default_rng(2)
    for t in range(3):
        eps = rng.standard_normal((B, 2, S, N, H, 1)).astype(np.float32)
        torch.manual_seed(40 + t)
        a_b, pw_b = batch.tick(states, pd, eps=eps)
        torch.manual_seed(40 + t)
        for e in range(B):
            lone[e].optimize(states[e], pd, eps=eps[e])
        outs = [lone[e].forward(states[e], pd) for e in range(B)]
        for e in range(B):
            assert elemerr(a_b[e].numpy(), outs[e][0].numpy()) < 25 * TOL and float((pw_b[e] - outs[e][1]).abs().max()) < 2e-3, (t, e)
            assert elemerr(batch.theta[e].numpy(), lone[e].theta.numpy()) < 25 * TOL, (t, e)
        if t == 0:
            batch, lone = copy.deepcopy(batch), [copy.deepcopy(o) for o in lone]
        for e in range(B):  # first-divergence form: the lone objects take the batch's particles over
            lone[e].theta = batch.theta[e]
    assert tuple(batch.theta.shape) == (B, N, H, 1)


def test_example_runs_three_periods():
    path = os.path.join(ROOT, "examples", "svmpc_batch_example.py")
    spec = importlib.util.spec_from_file_location("svmpc_batch_example", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    avg = mod.run(n_envs=4, steps=3, quiet=True)
    assert tuple(avg.shape) == (4,) and bool(torch.isfinite(avg).all()) and len(set(avg.tolist())) == 4
