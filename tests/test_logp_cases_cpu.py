"""The product-form float64 restatement of log p on large aliased sets (tests/logp_cases.py) is itself pinned, on the CPU: against the
exact-difference prior_ref of tests/pairwise_cases.py at 1e-10 (every case with N <= 2304 in full, 64 seeded rows of every larger one), its
far-block criterion against a pair-by-pair restatement; and - per case of tests/test_gpu_logp_sizes.py - it yields the tolerance the device
is held to (capped at 2e-4), the float64 far share of the islands inputs (0.05 ... 0.9) and the distance of every wrong variant (>= 10 tol)
("log p on large aliased sets at every compiled width").  Nothing here is computed from device output.
"""
import numpy as np
import pytest

import logp_cases as Q
import pairwise_cases as P

PIN_TOL = 1e-10


def _prior_ref_rows(theta, mix, sigma_p, rows):
    """prior_ref's log p (exact differences, float64) for the query rows `rows` against ALL keys: prior_ref takes as many means as
    particles, so the keys go through it in blocks of len(rows) with the block's share exp(log_mix) of the mixture as its weights
    (clamp=False: they are used as given), and the blocks' results are joined by a log-sum-exp."""
    N, B = theta.shape[0], len(rows)
    lm = P.log_mix(mix)
    parts = []
    for j0 in range(0, N, B):
        keys = np.minimum(np.arange(j0, j0 + B), N - 1)
        w = np.exp(lm[keys])
        w[np.arange(j0, j0 + B) >= N] = 0.0  # (the last block is filled up with weightless copies of the last key)
        with np.errstate(divide="ignore"):
            parts.append(P.prior_ref(theta[rows], theta[keys], w, sigma_p=sigma_p, clamp=False)[1] + np.log(w.sum()))
    parts = np.stack(parts)
    m = parts.max(0)
    return m + np.log(np.exp(parts - m).sum(0))


@pytest.mark.parametrize("case", Q.ALL_CASES, ids=lambda c: c["id"])
def test_logp_ref_vs_exact_differences(case):
    inp = Q.case_inputs(case)
    th, mix, sp = inp["theta"], inp["mix"], inp["sigma_p"]
    ref = Q.measure(case["id"])["ref"]
    assert np.isfinite(ref).all()
    if case["N"] <= Q.SMALL_N:
        err = float(np.abs(ref - P.prior_ref(th, th, mix, sigma_p=sp)[1]).max())
    else:
        rows = np.sort(np.random.default_rng(case["seed"] + 3).permutation(case["N"])[:64])
        err = float(np.abs(ref[rows] - _prior_ref_rows(th, mix, sp, rows)).max())
    print("%s: |logp_ref - prior_ref|max %.1e" % (case["id"], err))
    assert err < PIN_TOL, (case["id"], err)


def test_prior_ref_rows_is_prior_ref():
    """the row-subset form above against the whole prior_ref at a small case, ragged last key block, exact-zero weights"""
    case = Q.case_by_id("pend-N2049-D17-islands-zeros")
    inp = Q.case_inputs(case)
    rows = np.sort(np.random.default_rng(5).permutation(case["N"])[:64])
    full = P.prior_ref(inp["theta"], inp["theta"], inp["mix"], sigma_p=inp["sigma_p"])[1]
    assert float(np.abs(_prior_ref_rows(inp["theta"], inp["mix"], inp["sigma_p"], rows) - full[rows]).max()) < 1e-12


def test_live_blocks_vs_brute_force():
    """the criterion from exact differences, pair by pair: the two may differ only where a term sits within 1e-9 nats of the line"""
    case = Q.case_by_id("pend-N2111-D16-islands-steep")
    inp = Q.case_inputs(case)
    live = Q.measure(case["id"])["live"]
    assert live.shape == (33, 33)
    lo = Q.live_blocks_brute(inp["theta"], inp["mix"], inp["sigma_p"], Q.FAR_NATS - 1e-9)
    hi = Q.live_blocks_brute(inp["theta"], inp["mix"], inp["sigma_p"], Q.FAR_NATS + 1e-9)
    assert (live | ~lo).all() and (hi | ~live).all()
    assert 0 < (~live).sum() < live.size and live.diagonal().all()


@pytest.mark.parametrize("case", Q.ALL_CASES, ids=lambda c: c["id"])
def test_case_conditions(case):
    """the tolerance cap, the far share and the power of the variants - met by the choice of seeds and parameters in logp_cases.py"""
    m = Q.measure(case["id"])
    app = Q.logp_variants(case)
    print("%s [dpb %d]: |log p|max %.1f d_moved %.1e d_prod %.1e tol %.2e%s far share %.3f; variants / tol: %s; not applicable: %s" % (
        case["id"], case["dpb"], m["absmax"], m["d_moved"], m["d_prod"], m["tol"],
        " d32 %.1e tol_exact %.2e" % (m["d32"], m["tol_exact"]) if "d32" in m else "", m["far_share"],
        " ".join("%s %.0f" % (v, p / m["tol"]) for v, p in m["power"].items()), sorted(set(m["power"]) - set(app))))
    tols = [m["tol"]] + ([m["tol_exact"]] if "tol_exact" in m else [])
    assert max(tols) <= Q.TOL_CAP, tols
    if case["family"] == "islands":
        assert 0.05 <= m["far_share"] <= 0.9, m["far_share"]
    elif case["family"] == "dense":
        assert m["far_share"] == 0.0
    else:  # two clusters: the two off-diagonal quarters, up to the blocks that hold the boundary
        assert 0.45 <= m["far_share"] <= 0.5, m["far_share"]
    assert "drop_chunk" in app and len(app) >= 2
    if case["weights"] != "flat":
        assert "uniform_mix" in app
    if case["da"] == 2:
        assert "swap_sigma" in app
    for v in app:
        assert m["power"][v] >= 10 * max(tols), (case["id"], v, m["power"][v], max(tols))
    for v, why in Q.NOT_APPLICABLE.get(case["id"], {}).items():
        assert m["power"][v] < 10 * max(tols), "%s: %s is listed as not applicable (%s) but lies %.1e away" % (case["id"], v, why, m["power"][v])


def test_case_table_covers_every_width():
    """every row width the log-p kernels are compiled for, at a ragged N and at 2048 below the run-list threshold and at 8192 or 8193 / 8255
    above it; every D of the issue's list; Pendulum with an even D; the sizes 2048, 2049, 2111, 2304, 8192, 8193, 8255, ~12300, 16384"""
    for dpb in (16, 32, 48, 64, 80):
        assert any(c["dpb"] == dpb and c["N"] == 2048 for c in Q.SMALL_CASES)
        assert any(c["dpb"] == dpb and c["N"] in (2049, 2111) for c in Q.SMALL_CASES)
        assert any(c["dpb"] == dpb and c["N"] in (8192, 8193, 8255) for c in Q.LARGE_CASES)
        assert any(c["dpb"] == dpb and c["imq"] for c in Q.LARGE_CASES)
    assert {c["D"] for c in Q.ALL_CASES} >= {16, 17, 32, 33, 48, 49, 64, 65, 80}
    assert any(c["model"] == "pendulum" and c["D"] % 2 == 0 for c in Q.ALL_CASES)
    assert {c["N"] for c in Q.ALL_CASES} >= {2048, 2049, 2111, 2304, 8192, 8193, 8255, 16384}
    assert any(12200 <= c["N"] <= 12400 for c in Q.ALL_CASES)
    for fam in ("dense", "clusters"):
        assert any(c["family"] == fam for c in Q.SMALL_CASES) and any(c["family"] == fam for c in Q.LARGE_CASES)
