"""The K1 / IMQ Stein pass and the mixture-prior pass of every implementation against float64 restatements on DENSE clouds at tile edges
("K1 / IMQ and the prior beyond the fixtures").  The independent side is tests/pairwise_cases.py - plain float64 numpy
with exact differences, pinned on the CPU by tests/test_pairwise_cases_cpu.py.  Every tolerance is pairwise_cases.tolerances(case): max(1e-5,
2 d) <= 5e-5 for phi and grad_pri, max(2e-6 (1 + |log p|max), 2 d_abs) for log p, with d measured from the restatements alone (never from
device output).  One parametrised test per implementation:

| implementation | reached by | path on record |
| pairwise_kernel<PRIOR / LOGP / K1 / IMQ, CPT> (stein.hpp) | svmpc_phi on given costs and actions; optimize + forward for log p, with
|   DUST_LOGP_MFMA=0 and the default | profile slots pairwise_kernel<PRIOR> / <STEIN> in a second, profiled call (the slots name the ROLE:
|   which template instance serves it follows from D and, against pairwise_big_kernel, from the switch alone) |
| pairwise_big_kernel<., 32 / 64> (pairwise_big.hpp) | the same under DUST_PAIR_BIG=1 | as above; only the switch selects the kernel |
| pairwise_packed_kernel + pairwise_fused.hpp (+ pairwise_far.hpp) | DUST_PAIR_BIG=1, one tick to alias the prior, optimize(state, 1) |
|   no counter: the aliased prior (asserted) and the switch select the path |
| svmpc_tick2_kernel (tick2.hpp) | aliased state, optimize(state, 1) | tick_stats()["tick2"] rises by 1, "replayed" stays 0 |
| fused.hpp / the plain chain | the same under DUST_NO_TICK2=1 / DUST_NO_FUSE=1 | tick_stats()["tick2"] stays; plain chain: profile slots |
| svmpc_batch_kernel | Context.svmpc_batch(3), the case in slot 1 | profile slot svmpc_batch_kernel in a second, profiled call |

The whole-iteration forms (last four rows) are compared STAGE-WISE on the device's own inputs: the particles are read before the call;
grad_pri is held to prior_ref at those particles, phi to stein_ref at the DEVICE score, the new particles to the SGD step of the DEVICE phi
at 1e-6.  Each asserts on the particles it feeds the reference that the median K1 row mass is >= min(N, 8) / 2 and that every applicable
wrong variant of the restatement lies >= 10 tol away.  Environment switches are set before the context is created (read once, at create).
"""
import numpy as np
import pytest

import pairwise_cases as P
from helpers import elemerr

pytestmark = pytest.mark.gpu
STATE = {"pendulum": [3.0, 0.0], "particle": [-9.0, -9.0, 0.0, 0.0]}
ALPHA = {"pendulum": 1e-2, "particle": 1e-4}
LR = 1e-3
SGD_TOL = 1e-6


def _ctx(case, inp, S, sigma_a, **kw):
    from dust_amd import Context
    from oracle import grid_4x4_map  # data only (the demo's occupancy grid)

    model = case["model"]
    kw = dict(dict(model=model, N=case["N"], S=S, M=1, H=case["H"], kernel=case["kind"], imq_ell=P.IMQ_ELL, lr=LR, alpha=ALPHA[model],
                   sigma_a=sigma_a, sigma_p=inp["sigma_p"], weighted_prior=bool(case.get("weighted"))), **kw)
    if case["cov"] == "full":
        kw["p_cov"] = P.case_p_cov(case)
    c = Context(grid=grid_4x4_map() if model == "particle" else None, **kw)
    c.set_theta(inp["theta"])
    c.set_prior(inp["mu"], inp["mix"])
    c.set_a_mat(inp["theta"])
    return c


def _prior_kw(case, inp, c):
    """the prior scale as the context holds it: the full-covariance factor is read from the context (torch factors it in fp32)"""
    if case["cov"] == "full":
        return dict(chol_p=np.array([c.cfg.chol_p[0], c.cfg.chol_p[1], c.cfg.chol_p[2]], np.float32))
    return dict(sigma_p=inp["sigma_p"])


def _check(case, what, err, tol):
    print("%s [%s]: %s err %.2e (tol %.1e)" % (case["id"], case["dev"], what, err, tol))
    assert err < tol, "%s: %s err %.3e, tol %.1e" % (case["id"], what, err, tol)


def _power(case, what, dist, tol):
    for v, p in dist.items():
        assert p >= 10 * tol, "%s: %s variant %s is only %.2e from the reference (10 tol = %.1e)" % (case["id"], what, v, p, 10 * tol)


# ------------------------------------------------------------------------------------------------ the launch-per-stage pairwise kernels
def _pairwise_stage_test(case, monkeypatch):
    tol_phi, tol_pri, tol_logp = P.tolerances(case)
    inp = P.case_inputs(case)
    th, mu, mix = inp["theta"], inp["mu"], inp["mix"]
    N, H, da, S, sigma_a = case["N"], case["H"], case["da"], 8, 0.5
    rng = np.random.default_rng(case["seed"] + 2)
    actions = (th[None] + np.float32(sigma_a) * rng.standard_normal((S, N, H, da)).astype(np.float32)).astype(np.float32)
    costs = rng.uniform(0.0, 3.0 / ALPHA[case["model"]], (S, N)).astype(np.float32)
    state = np.array(STATE[case["model"]], np.float32)
    c = _ctx(case, inp, S, sigma_a)
    kw = _prior_kw(case, inp, c)
    phi, gl, gp = c.svmpc_phi(costs, actions)
    score = c.get_score()
    g_ref, _ = P.prior_ref(th, mu, mix, **kw)
    _check(case, "grad_pri", elemerr(gp, g_ref), tol_pri)
    d_lik, tol_lik = P.score_tolerance(th, mu, mix, costs, actions, ALPHA[case["model"]], sigma_a, case["seed"], lik_only=True, **kw)
    assert tol_lik <= P.TOL_CAP, d_lik
    _check(case, "grad_lik", elemerr(gl, P.lik_ref(th, costs, actions, ALPHA[case["model"]], sigma_a)), tol_lik)
    _check(case, "score = grad_lik + grad_pri", elemerr(score, np.asarray(gl, np.float64) + np.asarray(gp, np.float64)), 1e-6)
    _check(case, "phi", elemerr(phi, P.stein_ref(th, score, case["kind"], case["ell"])), tol_phi)
    ln = P.log_norm(H, da, **kw)
    for mfma in (None, "0"):  # log p of the forward pass (the prior pass without the gradient), both of its forms
        if mfma is not None:
            c.close()
            monkeypatch.setenv("DUST_LOGP_MFMA", mfma)
            c = _ctx(case, inp, S, sigma_a)
        c.svmpc_optimize(state, 1)
        th1 = c.get_theta()
        c.svmpc_forward()
        _, lp = c.get_log_weights()
        _, lp_ref = P.prior_ref(th1, mu, mix, **kw)
        _check(case, "log p (DUST_LOGP_MFMA=%s)" % mfma, float(np.abs(np.asarray(lp, np.float64) - (lp_ref + ln)).max()), tol_logp)
    # which launches served a call: a second, profiled svmpc_phi (profiling switches the launch fusions off: not the compared run)
    c.set_theta(th)
    c.profile(True)
    c.svmpc_phi(costs, actions)
    names = c.profile_get()
    c.close()
    assert "pairwise_kernel<PRIOR>" in names and "pairwise_kernel<STEIN>" in names, names


@pytest.mark.parametrize("case", P.PAIR_CASES, ids=lambda c: c["id"])
def test_pairwise_kernel_vs_float64(case, monkeypatch):
    """`pairwise_kernel<MODE, CPT>` (stein.hpp: 32-query tiles, 64-key chunks, key slices of pair_geometry) on a non-aliased prior:
    single-chunk slices up to N = 1024, two- and four-chunk slices beyond, N = 1025 with a last slice of one key, every CPT instance,
    Pendulum and Particle (two prior scales), IMQ, the full 2 x 2 prior covariance (whiten_rows_kernel), zero mixture weights over the
    whole first chunk, a centre of 50."""
    monkeypatch.setenv("DUST_PAIR_BIG", "0")
    _pairwise_stage_test(case, monkeypatch)


@pytest.mark.parametrize("case", P.BIG_CASES, ids=lambda c: c["id"])
def test_pairwise_big_kernel_vs_float64(case, monkeypatch):
    """`pairwise_big_kernel<MODE, 32 / 64>` (pairwise_big.hpp, query tiles of 128 / 64) under DUST_PAIR_BIG=1 on a non-aliased prior; only
    the switch selects the kernel (no counter tells it from pairwise_kernel)."""
    monkeypatch.setenv("DUST_PAIR_BIG", "1")
    _pairwise_stage_test(case, monkeypatch)


# ------------------------------------------------------------------------------------------------ the whole-iteration forms
def _aliased_iteration(case, monkeypatch, env, S, sigma_a=0.04):
    """One tick to alias the prior, then ONE optimize() iteration on device-drawn noise; returns what the stage-wise checks need.
    Small lr and sigma_a: the cloud stays dense, and grad_lik - a mean of S draws over sigma_a - is of the order of the 2 N(0, 1) stand-in
    the power of stale_score was measured with (at sigma_a = 0.1 the score is half that and the variant 8 tol away at N = 1000)."""
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    tol_phi, tol_pri, _ = P.tolerances(case)
    inp = P.case_inputs(case)
    state = np.array(STATE[case["model"]], np.float32)
    c = _ctx(case, inp, S, sigma_a, seed=case["seed"])
    c.svmpc_tick(state, 1)
    th, (mu1, mix) = c.get_theta(), c.get_prior()
    assert np.array_equal(mu1, th), "the prior means must alias the particles"
    assert P.dense_enough(th), "%s: median K1 row mass %.2f" % (case["id"], P.median_mass(th))
    before = c.tick_stats()
    c.svmpc_optimize(state, 1)
    after = c.tick_stats()
    (gl, gp), score, phi, th1 = c.get_score_parts(), c.get_score(), c.get_phi(), c.get_theta()
    assert np.isfinite(score).all() and float(np.abs(score).max()) > 0
    # grad_pri at the device's particles and mixture weights
    pv = tuple(v for v in P.prior_variants(case) if v != "uniform_mix" or case.get("weighted"))
    pr = P.prior_all(th, th, mix, sigma_p=inp["sigma_p"], variants=pv)
    _check(case, "grad_pri", elemerr(gp, pr[None][0]), tol_pri)
    _power(case, "grad_pri", {v: elemerr(pr[v][0], pr[None][0]) for v in pv}, tol_pri)
    # phi at the device's score
    st = P.stein_all(th, score, case["kind"], case["ell"], variants=P.stein_variants(case))
    _check(case, "phi", elemerr(phi, st[None]), tol_phi)
    _power(case, "phi", {v: elemerr(st[v], st[None]) for v in P.stein_variants(case)}, tol_phi)
    # the optimiser step at the device's phi
    _check(case, "theta_after", elemerr(th1, np.asarray(th, np.float64) + float(np.float32(LR)) * np.asarray(phi, np.float64)), SGD_TOL)
    return c, before, after


@pytest.mark.parametrize("case", P.FUSEDBIG_CASES, ids=lambda c: c["id"])
def test_fused_large_set_pass_vs_float64(case, monkeypatch):
    """pairwise_fused.hpp + pairwise_packed.hpp (+ pairwise_far.hpp) under DUST_PAIR_BIG=1 with an aliased prior: one distance pass for the
    prior score, the repulsion and the Gram matrix, then Gram x score.  Default far threshold and DUST_FAR=0; on a dense cloud nothing is
    far; the two-cluster case has whole far units next to dense near ones.  No counter names this path: the aliased prior (asserted)
    and the switch select it."""
    env = {"DUST_PAIR_BIG": "1"}
    if case["far"] == "0":
        env["DUST_FAR"] = "0"
    c, _, _ = _aliased_iteration(case, monkeypatch, env, S=8)
    c.close()


@pytest.mark.parametrize("case", P.TICK2_CASES, ids=lambda c: c["id"])
def test_tick2_vs_float64(case, monkeypatch):
    """`svmpc_tick2_kernel` (tick2.hpp): N % 4 == 0 but no multiple of 32 or 64 (ragged key chunks and owner groups), one dimension, the full
    row of 32, Particle with H = 1 and 16, IMQ, non-uniform mixture weights (weighted_prior).  tick_stats()["tick2"] rises by one."""
    c, before, after = _aliased_iteration(case, monkeypatch, {}, S=64)
    c.close()
    assert after["tick2"] == before["tick2"] + 1 and after["replayed"] == 0, (before, after)


@pytest.mark.parametrize("case", P.FUSED_CASES, ids=lambda c: c["id"])
def test_fused_launches_vs_float64(case, monkeypatch):
    """fused.hpp (`fused_prior_rollout_kernel`, `stein_update_kernel`, `svgd_iter_kernel`) under DUST_NO_TICK2=1, and the plain launch chain
    under DUST_NO_FUSE=1.  No counter names the fused launches (only the switch selects them; tick_stats()["tick2"] must stay); the plain
    chain shows its launches in a second, profiled iteration."""
    env = {"DUST_NO_TICK2": "1"} if case["path"] == "nofuse" else {"DUST_NO_FUSE": "1"}
    c, before, after = _aliased_iteration(case, monkeypatch, env, S=64)
    assert after["tick2"] == before["tick2"] == 0, (before, after)
    if case["path"] == "plain":
        c.profile(True)
        c.svmpc_optimize(np.array(STATE[case["model"]], np.float32), 1)
        names = c.profile_get()
        assert "pairwise_kernel<PRIOR>" in names and "pairwise_kernel<STEIN>" in names, names
    c.close()


@pytest.mark.parametrize("case", P.BATCH_CASES, ids=lambda c: c["id"])
def test_svmpc_batch_kernel_vs_float64(case):
    """`svmpc_batch_kernel` (svmpc_batch.hpp): the case in slot 1 of three environments, other clouds in slots 0 and 2, non-aliased prior
    with non-uniform weights.  The batch records the score, not its parts: it is held to lik_ref (at the device's costs and kept
    actions) + prior_ref; phi to stein_ref at the device's score; log p after forward().  A second, profiled call shows the
    svmpc_batch_kernel slot."""
    from dust_amd import _lib as L

    tol_phi, tol_pri, tol_logp = P.tolerances(case)
    inp = P.case_inputs(case)
    sides = [P.case_inputs(dict(case, seed=case["seed"] + k)) for k in (1, 2)]
    three = lambda q: np.stack([sides[0][q], inp[q], sides[1][q]])
    model, N, H, da, S, sigma_a = case["model"], case["N"], case["H"], case["da"], 16, 2.0
    # (alpha: a tenth of the other rows' for Pendulum - its costs grow with H, and at H = 128 and alpha = 1e-2 the rounding of alpha * cost
    #  alone puts score_tolerance's d at 3e-5 ... 5e-5, beyond the cap)
    alpha = ALPHA[model] * (0.1 if model == "pendulum" else 1.0)
    proto = _ctx(case, inp, S, sigma_a, seed=case["seed"], alpha=alpha)
    b = proto.svmpc_batch(3)
    b.set(L.SVB_THETA, three("theta"))
    b.set(L.SVB_PRIOR_MEANS, three("mu"))
    b.set(L.SVB_PRIOR_MIX, three("mix"))
    b.set(L.SVB_A_MAT, three("theta"))
    states = np.stack([np.array(STATE[model], np.float32)] * 3)
    th, mu, mix = inp["theta"], inp["mu"], b.get(L.SVB_PRIOR_MIX)[1]
    assert P.dense_enough(th), P.median_mass(th)
    b.optimize(states, 1, keep_actions=True)
    score, phi, th1 = b.get(L.SVB_SCORE)[1], b.get(L.SVB_PHI)[1], b.get(L.SVB_THETA)[1]
    costs, actions = b.get(L.SVB_COSTS)[1], b.get(L.SVB_ACTIONS)[1]
    kw = dict(sigma_p=inp["sigma_p"])
    s_ref = P.lik_ref(th, costs, actions, alpha, sigma_a) + P.prior_ref(th, mu, mix, **kw)[0]
    d_sc, tol_sc = P.score_tolerance(th, mu, mix, costs, actions, alpha, sigma_a, case["seed"], **kw)
    assert tol_sc <= P.TOL_CAP, d_sc
    _check(case, "score (d %.1e)" % d_sc, elemerr(score, s_ref), tol_sc)
    st = P.stein_all(th, score, case["kind"], case["ell"], variants=P.stein_variants(case))
    _check(case, "phi", elemerr(phi, st[None]), tol_phi)
    _power(case, "phi", {v: elemerr(st[v], st[None]) for v in P.stein_variants(case)}, tol_phi)
    _check(case, "theta_after", elemerr(th1, np.asarray(th, np.float64) + float(np.float32(LR)) * np.asarray(phi, np.float64)), SGD_TOL)
    b.forward()
    lp = b.get(L.SVB_LOG_P)[1]
    _check(case, "log p", float(np.abs(np.asarray(lp, np.float64) - (P.prior_ref(th1, mu, mix, **kw)[1] + P.log_norm(H, da, **kw))).max()), tol_logp)
    b.ctx.profile(True)
    b.optimize(states, 1)
    names = b.ctx.profile_get()
    b.close()
    proto.close()
    assert "svmpc_batch_kernel" in names, names
