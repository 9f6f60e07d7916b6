"""Owner-computes one-launch tick (dust_amd/csrc/tick2.hpp) against the launch-per-iteration paths (DUST_NO_TICK2: the fused launch
forms; the tiled one-launch tick of rounds 2-5, persist.hpp, is retired) and the CPU oracle.  The reference path is `optimize(); forward()` of dust/utils/simulations.py:104-123
(SVMPC.optimize svmpc.py:97-126, SVMPC.forward svmpc.py:172-200).  tick2 takes a tick when the prior means alias the particles
(every tick after the first forward), N % 4 == 0, N <= 1024, H * d_a <= 32; `tick_stats()` tells which path served a call."""
import os

import numpy as np
import pytest

from helpers import elemerr

pytestmark = pytest.mark.gpu

TOL = 2e-5  # element-wise (|a - b| / (|b| + rms b)): sums over keys / samples are taken in another order than in the tiled kernels


def _state(model):
    return np.array([3.0, 0.0], np.float32) if model == "pendulum" else np.array([-9.0, -9.0, 0.0, 0.0], np.float32)


def _make(model, N, S, H, M=1, kernel="K1", optimizer="SGD", seed=0, weighted_prior=False, roll="repeat", lik=None):
    from dust_amd import Context

    da = 1 if model == "pendulum" else 2
    rng = np.random.default_rng(seed)
    mu = rng.standard_normal((N, H, da)).astype(np.float32)
    th = (mu + 2 * rng.standard_normal((N, H, da))).astype(np.float32)
    kw = {}
    if model == "particle":
        from oracle import grid_4x4_map

        kw["grid"] = grid_4x4_map()
        if M > 1:
            kw["uncertain_params"] = ("mass",)
    elif M > 1:
        kw["uncertain_params"] = ("length", "mass")
    if lik:
        kw["likelihood"] = lik
    sig = 2.0 if model == "pendulum" else 5.0
    c = Context(model=model, N=N, S=S, M=M, H=H, kernel=kernel, lr=2.0 if model == "pendulum" else 100.0, sigma_a=sig, sigma_p=sig,
                optimizer=optimizer, weighted_prior=weighted_prior, roll_strategy=roll, seed=77, **kw)
    c.set_theta(th)
    c.set_prior(mu)
    c.set_a_mat(th)
    return c, rng


def _snapshot(c):
    ll, lp = c.get_log_weights()
    return dict(theta=c.get_theta(), a_mat=c.get_a_mat(), costs=c.get_costs(), score=c.get_score(), phi=c.get_phi(), ll=ll, lp=lp,
                mix=c.get_prior()[1])


def _run(env, model, N, S, H, iters, ticks, ext_noise, M=1, **kw):
    saved = {k: os.environ.pop(k, None) for k in ("DUST_NO_TICK2",)}
    os.environ.update(env)
    try:
        c, rng = _make(model, N, S, H, M=M, **kw)
        da = 1 if model == "pendulum" else 2
        st = _state(model)
        outs = []
        for t in range(ticks):
            eps = rng.standard_normal((iters, S, N, H, da)).astype(np.float32) if ext_noise else None
            params = None
            if M > 1:
                P = 1 if model == "particle" else 2
                params = (1.0 + 0.1 * rng.standard_normal((iters, M, P))).astype(np.float32)
            a_seq, pw = c.svmpc_tick(st, iters, eps=eps, params=params)
            outs.append(dict(a_seq=a_seq.copy(), pw=pw.copy(), **_snapshot(c)))
        stats = c.tick_stats()
        c.close()
        return outs, stats
    finally:
        for k in ("DUST_NO_TICK2",):
            os.environ.pop(k, None)
            if saved[k] is not None:
                os.environ[k] = saved[k]


SHAPES = [
    # model, N, S, H, iters, M, kw
    ("pendulum", 64, 128, 15, 3, 1, {}),
    ("pendulum", 1024, 128, 30, 5, 1, {}),                      # BASELINE configs[1]
    ("pendulum", 128, 128, 30, 2, 1, dict(kernel="IMQ")),
    ("pendulum", 96, 64, 20, 3, 1, dict(optimizer="Adam")),      # N not a multiple of 64: masked keys; S = 64: one wave per particle
    ("pendulum", 64, 96, 12, 2, 4, {}),                          # sampled dynamics (length, mass), S not a multiple of 64
    ("pendulum", 256, 128, 30, 2, 1, dict(weighted_prior=True)),
    ("pendulum", 64, 128, 16, 2, 1, dict(roll="mean")),
    ("pendulum", 64, 128, 16, 2, 1, dict(lik="ExpectedCost")),
    ("particle", 64, 64, 12, 2, 1, {}),
    ("particle", 128, 64, 16, 2, 4, dict(kernel="IMQ")),
]


def _make_with_env(env, *a, **kw):
    """a context created under the given development switches (the library reads them once, at dust_create)"""
    saved = {k: os.environ.pop(k, None) for k in ("DUST_NO_TICK2",)}
    os.environ.update(env)
    try:
        return _make(*a, **kw)
    finally:
        for k in ("DUST_NO_TICK2",):
            os.environ.pop(k, None)
            if saved[k] is not None:
                os.environ[k] = saved[k]


@pytest.mark.parametrize("ext_noise", [True, False])
@pytest.mark.parametrize("model,N,S,H,iters,M,kw", SHAPES)
def test_tick2_equals_launch_per_iteration(model, N, S, H, iters, M, kw, ext_noise):
    """Three ticks of two contexts side by side: tick 1 runs plain kernels on both (the prior means do not alias the particles yet),
    ticks 2-3 run tick2.hpp in one and the launch-per-iteration forms in the other.  Caller-supplied noise and the device Philox stream (same counter
    layout in both kernels).  After every tick the other context takes over the owner-computes context's particles, a_mat and mixture,
    so EVERY tick is a first-divergence comparison at the tolerances of one tick (round 3 let the two runs drift apart and compared
    the third tick at 2e-2, which proved little - VERDICT r3): costs at 2e-5 element-wise, what lies downstream of
    exp(-alpha cost) - one ulp of a cost of 1e3 is 1e-4 on a weight - at 5e-4."""
    a, rng_a = _make_with_env({}, model, N, S, H, M=M, **kw)
    b, rng_b = _make_with_env({"DUST_NO_TICK2": "1"}, model, N, S, H, M=M, **kw)
    da = 1 if model == "pendulum" else 2
    st = _state(model)
    for t in range(3):
        eps = rng_a.standard_normal((iters, S, N, H, da)).astype(np.float32) if ext_noise else None
        params = None
        if M > 1:
            params = (1.0 + 0.1 * rng_a.standard_normal((iters, M, 1 if model == "particle" else 2))).astype(np.float32)
        ra = a.svmpc_tick(st, iters, eps=eps, params=params)
        rb = b.svmpc_tick(st, iters, eps=eps, params=params)
        sa, sb = dict(a_seq=ra[0], pw=ra[1], **_snapshot(a)), dict(a_seq=rb[0], pw=rb[1], **_snapshot(b))
        for k in ("costs", "score", "phi", "theta", "a_mat", "ll", "lp", "a_seq"):
            tol = TOL * (25 if k in ("score", "phi", "theta", "a_mat", "a_seq", "ll") else 1)
            assert elemerr(sa[k], sb[k]) < tol, (t, k, elemerr(sa[k], sb[k]))
        assert np.abs(sa["pw"] - sb["pw"]).max() < 2e-3, t
        b.set_theta(a.get_theta())  # (the prior means alias the particles: they follow)
        b.set_a_mat(a.get_a_mat())
        if kw.get("weighted_prior"):
            b.svmpc_update_prior(ra[1])
            a.svmpc_update_prior(ra[1])
    stats_a, stats_b = a.tick_stats(), b.tick_stats()
    a.close()
    b.close()
    assert stats_a["tick2"] == 2 and stats_a["replayed"] == 0, stats_a
    assert stats_b["tick2"] == 0, stats_b


def test_tick2_optimize_only_then_forward():
    """SVMPC.optimize alone (particles and Adam state stay, svmpc.py:97-126) followed by a separate forward: both through tick2."""
    res = []
    for env in ({}, {"DUST_NO_TICK2": "1"}):
        saved = os.environ.pop("DUST_NO_TICK2", None)
        os.environ.update(env)
        try:
            c, rng = _make("pendulum", 64, 128, 15, optimizer="Adam")
            st = _state("pendulum")
            eps = rng.standard_normal((3, 128, 64, 15, 1)).astype(np.float32)
            c.svmpc_tick(st, 1, eps=eps[:1])          # aliases the prior
            c.svmpc_optimize(st, 2, eps=eps[1:])      # two Adam steps, no forward
            th_mid = c.get_theta()
            a_seq, pw = c.svmpc_forward()
            res.append((th_mid, a_seq, pw, c.get_theta(), c.tick_stats()))
            c.close()
        finally:
            os.environ.pop("DUST_NO_TICK2", None)
            if saved is not None:
                os.environ["DUST_NO_TICK2"] = saved
    (t0, a0, p0, e0, s0), (t1, a1, p1, e1, s1) = res
    assert s0["tick2"] >= 1 and s1["tick2"] == 0
    assert elemerr(t0, t1) < 1e-4 and elemerr(a0, a1) < 1e-4 and elemerr(e0, e1) < 1e-4
    assert np.abs(p0 - p1).max() < 2e-3


def test_tick2_against_oracle_whole_tick():
    """One whole tick (5 iterations + forward) at the product shape against the CPU oracle fed the same noise."""
    from oracle import Oracle

    N, S, H, K = 256, 128, 30, 3
    c, rng = _make("pendulum", N, S, H)
    st = _state("pendulum")
    eps0 = rng.standard_normal((1, S, N, H, 1)).astype(np.float32)
    c.svmpc_tick(st, 1, eps=eps0)  # tick 1 (plain kernels): afterwards the prior means alias the particles
    th, (mu, mix), am = c.get_theta(), c.get_prior(), c.get_a_mat()
    eps = rng.standard_normal((K, S, N, H, 1)).astype(np.float32)
    a_seq, pw = c.svmpc_tick(st, K, eps=eps)
    assert c.tick_stats()["tick2"] == 1
    o = Oracle(model="pendulum", N=N, S=S, M=1, H=H)
    r = o.tick_k1(st, th, th, mix, 2.0, 2.0, eps, K, 1.0, 2.0, am)
    # the tick's particles BEFORE the roll are not kept; compare the rolled particles and the chosen sequence
    assert elemerr(c.get_theta(), r["theta"]) < 2e-3, elemerr(c.get_theta(), r["theta"])
    assert np.abs(pw - r["p_weights"]).max() < 2e-3
    if np.sort(r["p_weights"])[-1] - np.sort(r["p_weights"])[-2] > 1e-2:
        assert elemerr(a_seq.reshape(-1), r["a_seq"].reshape(-1)) < 2e-3
    c.close()


def test_tick2_long_run_stays_consistent():
    """400 product ticks (device noise) through tick2 and through the launch-per-iteration forms from the same start: finite throughout, and the
    first 3 ticks - before chaos separates the two summation orders - agree."""
    N, S, H = 1024, 128, 30
    st = _state("pendulum")
    outs = []
    for env in ({}, {"DUST_NO_TICK2": "1"}):
        saved = os.environ.pop("DUST_NO_TICK2", None)
        os.environ.update(env)
        try:
            c, _ = _make("pendulum", N, S, H)
            hist = []
            for t in range(400):
                a_seq, pw = c.svmpc_tick(st, 5)
                if t < 3:
                    hist.append((a_seq.copy(), pw.copy()))
                assert np.isfinite(a_seq).all() and abs(float(pw.sum()) - 1.0) < 1e-3, t
            assert np.isfinite(c.get_theta()).all()
            outs.append((hist, c.tick_stats()))
            c.close()
        finally:
            os.environ.pop("DUST_NO_TICK2", None)
            if saved is not None:
                os.environ["DUST_NO_TICK2"] = saved
    (h0, s0), (h1, s1) = outs
    assert s0["tick2"] == 399 and s0["replayed"] == 0 and s1["tick2"] == 0
    for t in range(2):
        assert elemerr(h0[t][0], h1[t][0]) < 1e-3, t


def test_tick2_timed_out_ticks_commit_nothing_and_are_replayed():
    """A tick of the owner-computes kernel one of whose in-launch waits gives up (another PROCESS computing on the device:
    tools/two_process_ticks.py) writes no persistent state - particles, a_mat, optimiser moments, stream counters are committed
    behind the last wait under ONE verdict word - and is replayed by the library on plain kernels; afterwards the context stays off
    every kernel that spins on its own grid.  DUST_TICK2_TEST_TIMEOUT=3: the last workgroup of the third launch acts as if its last
    wait had given up."""
    N, S, H = 256, 128, 30
    st = _state("pendulum")
    outs = []
    for env in ({"DUST_TICK2_TEST_TIMEOUT": "3"}, {}):
        saved = os.environ.pop("DUST_TICK2_TEST_TIMEOUT", None)
        os.environ.update(env)
        try:
            c, _ = _make("pendulum", N, S, H)
            hist = []
            for t in range(7):
                a_seq, pw = c.svmpc_tick(st, 3)
                hist.append((a_seq.copy(), pw.copy(), c.get_theta()))
            outs.append((hist, c.tick_stats()))
            c.close()
        finally:
            os.environ.pop("DUST_TICK2_TEST_TIMEOUT", None)
            if saved is not None:
                os.environ["DUST_TICK2_TEST_TIMEOUT"] = saved
    (h0, s0), (h1, s1) = outs
    assert s0["tick2"] == 3 and s0["replayed"] == 1, s0   # launches 1-3 of the owner-computes kernel, then plain kernels for good
    assert s1["tick2"] == 6 and s1["replayed"] == 0, s1
    for t in range(5):  # t = 3 is the replayed tick; from then on the two runs sum in different orders, later ticks amplify
        assert elemerr(h0[t][0], h1[t][0]) < 2e-3, (t, elemerr(h0[t][0], h1[t][0]))
        assert np.abs(h0[t][1] - h1[t][1]).max() < 5e-3
        if t < 3:
            assert np.array_equal(h0[t][2], h1[t][2]), t
    for t in range(7):
        assert np.isfinite(h0[t][2]).all() and abs(float(h0[t][1].sum()) - 1.0) < 1e-3


def test_tick2_aborted_ticks_are_replayed():
    """A tick whose workgroups are not all resident does not start (start barrier) and is replayed by the library on the
    launch-per-iteration path: the caller sees DUST_OK, the same results, and `tick_stats()['replayed']` counts it.  The test hook
    DUST_TICK2_TEST_ABORT=3 makes workgroup 0 publish "abort" on every third launch."""
    N, S, H = 256, 128, 30
    st = _state("pendulum")
    outs = []
    for env in ({"DUST_TICK2_TEST_ABORT": "3"}, {}):
        saved = os.environ.pop("DUST_TICK2_TEST_ABORT", None)
        os.environ.update(env)
        try:
            c, _ = _make("pendulum", N, S, H)
            hist = []
            for t in range(8):
                a_seq, pw = c.svmpc_tick(st, 3)
                hist.append((a_seq.copy(), pw.copy(), c.get_theta()))
            outs.append((hist, c.tick_stats()))
            c.close()
        finally:
            os.environ.pop("DUST_TICK2_TEST_ABORT", None)
            if saved is not None:
                os.environ["DUST_TICK2_TEST_ABORT"] = saved
    (h0, s0), (h1, s1) = outs
    assert s0["tick2"] == 7 and s0["replayed"] == 2, s0   # launches 3 and 6 of the 7 owner-computes ticks
    assert s1["replayed"] == 0
    for t in range(4):  # the replayed tick (t = 3: third tick2 launch) sums in another order; later ticks amplify
        assert elemerr(h0[t][0], h1[t][0]) < 2e-3, (t, elemerr(h0[t][0], h1[t][0]))
        assert np.abs(h0[t][1] - h1[t][1]).max() < 5e-3
    for t in range(8):
        assert np.isfinite(h0[t][2]).all() and abs(float(h0[t][1].sum()) - 1.0) < 1e-3


@pytest.mark.parametrize("model,N,S,H,M,kernel,optimizer", [
    ("pendulum", 1024, 128, 30, 1, "K1", "SGD"),    # BASELINE configs[1], the shape bench.py times
    ("pendulum", 1024, 128, 30, 1, "K1", "Adam"),
    ("pendulum", 512, 128, 30, 1, "IMQ", "SGD"),
    ("particle", 256, 64, 16, 4, "K1", "SGD"),      # sampled dynamics (mass), occupancy grid in LDS
    ("particle", 256, 64, 16, 4, "IMQ", "Adam"),
])
def test_tick2_stage_parity_vs_oracle(model, N, S, H, M, kernel, optimizer):
    """the kernel the bench times, held to the ORACLE stage by stage at 1e-5.  From an aliased state one optimize()
    of ONE iteration through `svmpc_tick2_kernel` with caller-supplied noise: a one-iteration launch is stage-local - the costs depend
    on theta and eps only, the score on the costs, phi on the score - so every stage is compared with the oracle fed the stage before it
    (the policy of DESIGN.md section 2: one ulp of a cost of 1e3 is 1e-4 on a softmax weight).  Reference path: SVMPC.step svmpc.py:87-95
    -> likelihood.sample likelihoods.py:81-101 -> MultiDISCO._rollout / _compute_cost disco.py:139-346 -> SVMPC.phi svmpc.py:38-83.
    At these inputs (theta = mu + sigma N(0, 1), K1's lengthscale ln 2) the K1 Gram matrix is the IDENTITY - the largest off-diagonal
    row mass is 1e-30 - so phi_i = score_i / N whatever the kernel does with the other keys, and the aliased prior's responsibilities
    are the identity too: rollouts, costs, score and step are held here; the Stein and prior passes over a DENSE Gram matrix are held
    in tests/test_gpu_pairwise_sizes.py (test_pairwise_cases_cpu.py asserts this fact)."""
    from dust_amd import Context
    from oracle import Oracle, grid_4x4_map
    from test_oracle_golden import k1_tolerance

    da = 1 if model == "pendulum" else 2
    rng = np.random.default_rng(1234 + N + H)
    sig = 2.0 if model == "pendulum" else 5.0
    alpha = 1.0 if model == "pendulum" else 1e-4
    lr = 2.0 if model == "pendulum" else 100.0
    kw = {}
    P = 0
    if model == "particle":
        kw["grid"] = grid_4x4_map()
        kw["uncertain_params"] = ("mass",)
        P = 1
    mu = rng.standard_normal((N, H, da)).astype(np.float32)
    th0 = (mu + sig * rng.standard_normal((N, H, da))).astype(np.float32)
    c = Context(model=model, N=N, S=S, M=M, H=H, kernel=kernel, imq_ell=0.9, lr=lr, alpha=alpha, sigma_a=sig, sigma_p=sig,
                optimizer=optimizer, seed=5, **kw)
    c.set_theta(th0)
    c.set_prior(mu)
    c.set_a_mat(th0)
    st = _state(model)
    par = lambda: (1.0 + 0.1 * rng.standard_normal((1, M, P))).astype(np.float32) if P else None
    c.svmpc_tick(st, 1, eps=rng.standard_normal((1, S, N, H, da)).astype(np.float32), params=par())  # aliases the prior
    th, (mu1, mix), am = c.get_theta(), c.get_prior(), c.get_a_mat()
    assert np.array_equal(mu1, th)
    eps = rng.standard_normal((1, S, N, H, da)).astype(np.float32)
    params = par()
    before = c.tick_stats()["tick2"]
    c.svmpc_optimize(st, 1, eps=eps, params=params)
    assert c.tick_stats()["tick2"] == before + 1 and c.tick_stats()["replayed"] == 0, c.tick_stats()
    costs, (gl, gp), score, phi, th1 = c.get_costs(), c.get_score_parts(), c.get_score(), c.get_phi(), c.get_theta()
    c.close()

    o = Oracle(model=model, N=N, S=S, M=M, H=H, grid=kw.get("grid"), uncertain_params=kw.get("uncertain_params"))
    sv = np.full(da, sig, np.float32)
    actions = o.sample_actions(th, eps[0], sv)
    costs_ref = o.rollout_cost(st, actions, None if params is None else params[0])
    assert elemerr(costs, costs_ref) < 1e-5, elemerr(costs, costs_ref)                      # a1-a5: rollouts + costs
    gl_ref, gp_ref, sc_ref = o.score(th, th, mix, sv, costs, actions, alpha, sv)            # a9, fed the DEVICE costs
    assert elemerr(gl, gl_ref) < 1e-5 and elemerr(gp, gp_ref) < 1e-5, (elemerr(gl, gl_ref), elemerr(gp, gp_ref))
    assert elemerr(score, sc_ref) < 1e-5
    phi_ref = o.phi_k1(th, score) if kernel == "K1" else o.phi_imq(th, score, 0.9)          # a10 / IMQ, fed the DEVICE score
    assert elemerr(phi, phi_ref) < (k1_tolerance(th) if kernel == "K1" else 1e-5), elemerr(phi, phi_ref)
    if optimizer == "SGD":                                                                  # a8, fed the DEVICE phi
        th_ref = o.sgd(th, phi, lr)
    else:
        th_ref, _, _ = o.adam(th, phi, np.zeros_like(th), np.zeros_like(th), 1, lr)
    assert elemerr(th1, th_ref) < 1e-6, elemerr(th1, th_ref)


def test_tick2_open_loop_queue_aborts_in_order():
    """ticks enqueued WITHOUT reading their outputs, each with another plant state.  The third launch does not
    start (hook); every one-launch tick enqueued behind it must not run ahead of its replay - the kernels compare the device's abort
    count with the value the host knew at launch (`expect_aborts`) and abort too - and the library replays the whole tail in order,
    each tick with its own inputs.  Also: an optimize() that did not start followed by forward() - the forward stays behind it."""
    N, S, H = 256, 128, 30
    states = [np.array([3.0 - 0.4 * t, 0.2 * t], np.float32) for t in range(6)]
    outs = []
    for env in ({"DUST_TICK2_TEST_ABORT": "3"}, {}):
        saved = os.environ.pop("DUST_TICK2_TEST_ABORT", None)
        os.environ.update(env)
        try:
            c, _ = _make("pendulum", N, S, H)
            c.svmpc_tick(states[0], 2)                      # tiled form: aliases the prior
            for t in range(1, 6):                          # launches 1-5 of the owner-computes kernel, nothing read back in between
                c.svmpc_tick(states[t], 2, want_outputs=False)
            c.sync()
            th = c.get_theta()
            stats = c.tick_stats()
            # optimize() alone (launch 6: aborted by the hook in the first run) and a separate forward()
            c.svmpc_optimize(states[1], 2)
            a_seq, pw = c.svmpc_forward()
            outs.append((th, stats, a_seq, pw, c.get_theta(), c.tick_stats()))
            c.close()
        finally:
            os.environ.pop("DUST_TICK2_TEST_ABORT", None)
            if saved is not None:
                os.environ["DUST_TICK2_TEST_ABORT"] = saved
    (t0, s0, a0, p0, e0, f0), (t1, s1, a1, p1, e1, f1) = outs
    assert s0["replayed"] == 3 and s1["replayed"] == 0, (s0, s1)   # launch 3 did not start; launches 4 and 5 went with it
    assert f0["replayed"] == 5, f0                                   # launch 6 (the optimize) and the forward behind it
    assert elemerr(t0, t1) < 5e-3, elemerr(t0, t1)                   # (replays sum in another order; three ticks amplify)
    assert elemerr(e0, e1) < 2e-2 and np.abs(p0 - p1).max() < 2e-2
    assert np.isfinite(e0).all() and abs(float(p0.sum()) - 1.0) < 1e-3


@pytest.mark.parametrize("env", [{}, {"DUST_NO_TICK2": "1"}, {"DUST_NO_TICK2": "1"}], ids=["tick2", "fused-launches", "launch-per-iteration"])
def test_contexts_tick_concurrently(env):
    """Three contexts on one device ticking from three host threads.  Every one-launch form spins on its own
    workgroups and needs them co-resident; with a second context on the device the library chains those launches across the
    contexts' streams (and the owner-computes tick additionally proves residency at its start and is replayed otherwise).  No
    tick may be lost or fail: every call returns, results stay finite and normalised.  All tick forms: the owner-computes kernel, the
    fused launch-per-iteration forms with in-launch hand-offs, plain launches."""
    import threading

    N, S, H, T, C = 1024, 128, 30, 120, 3
    st = _state("pendulum")
    saved = {k: os.environ.pop(k, None) for k in ("DUST_NO_TICK2",)}
    os.environ.update(env)
    try:
        ctxs = [_make("pendulum", N, S, H, seed=s)[0] for s in range(C)]
        errs, stats = [], [None] * C

        def run(i):
            try:
                c = ctxs[i]
                for t in range(T):
                    a_seq, pw = c.svmpc_tick(st, 5)
                    assert np.isfinite(a_seq).all() and abs(float(pw.sum()) - 1.0) < 1e-3, (i, t)
                stats[i] = c.tick_stats()
            except Exception as e:  # noqa: BLE001
                errs.append((i, repr(e)))

        th = [threading.Thread(target=run, args=(i,)) for i in range(C)]
        for t in th:
            t.start()
        for t in th:
            t.join()
        assert not errs, errs
        for i in range(C):
            if not env:
                assert stats[i]["tick2"] == T - 1, stats[i]
            assert np.isfinite(ctxs[i].get_theta()).all()
            ctxs[i].close()
        print("replayed ticks:", [s["replayed"] for s in stats])
    finally:
        for k in ("DUST_NO_TICK2",):
            os.environ.pop(k, None)
            if saved[k] is not None:
                os.environ[k] = saved[k]

@pytest.mark.parametrize("model,N,S,H,iters,M,kw", [("pendulum", 2048, 16, 30, 2, 1, {}), ("pendulum", 2048, 16, 12, 2, 2, dict(kernel="IMQ")),
                                                    ("particle", 2048, 16, 16, 2, 1, {})])
def test_n2048_short_rows_default_path_equals_the_other_paths(model, N, S, H, iters, M, kw):
    """N = 2048 with N D <= 65 536 runs the small-set kernels by default since round 3 (dust_amd.hip pair_is_big) - whichever launch form
    that is for the shape (fused launches): the same two ticks through the launch-per-iteration kernels
    (DUST_NO_FUSE) and through the large-set path (DUST_PAIR_BIG=1, the default until then and the one the oracle tests of
    test_gpu_parity.py pin at this size) must agree."""
    outs = {}
    for name, env in (("default", {}), ("plain", {"DUST_NO_FUSE": "1"}), ("large", {"DUST_PAIR_BIG": "1"})):
        saved = {k: os.environ.pop(k, None) for k in ("DUST_PAIR_BIG", "DUST_NO_FUSE")}
        try:
            outs[name] = _run(env, model, N, S, H, iters, 2, True, M=M, **kw)
        finally:
            for k in ("DUST_PAIR_BIG", "DUST_NO_FUSE"):
                os.environ.pop(k, None)
                if saved[k] is not None:
                    os.environ[k] = saved[k]
    (a, sa), (b, _), (c, _) = outs["default"], outs["plain"], outs["large"]
    assert sa["tick2"] == 0, sa
    for other in (b, c):
        for t in range(2):
            for k in ("costs", "score", "phi", "theta", "a_mat", "ll", "lp", "a_seq"):
                # (different kernels from the first tick on: everything downstream of exp(-alpha cost) carries the summation order)
                tol = TOL * (25 if k in ("score", "phi", "theta", "a_mat", "a_seq", "ll") else 1) * (1 if t == 0 else 4)
                assert elemerr(a[t][k], other[t][k]) < tol, (t, k, elemerr(a[t][k], other[t][k]))
            assert np.abs(a[t]["pw"] - other[t]["pw"]).max() < 4e-3
    print("paths at N = 2048:", sa)
