"""The float64 restatement of the K2 Stein step (tests/k2_cases.py) is itself pinned, on the CPU: against the reference's own goldens on every
K2 fixture, against the oracle at sizes the fixtures do not reach, and - per case of tests/test_gpu_k2_sizes.py - it yields the tolerance
the device is held to and shows that each power variant lies at least ten tolerances away ("K2 beyond the fixtures").
"""
import numpy as np
import pytest

import k2_cases as K
from helpers import elemerr, k2_tolerance, relerr, scenario_kwargs
from oracle import Oracle
from test_oracle_golden import _prior_at, _sig

K2_FIXTURES = ["pend_k2", "part_k2_gmm", "part_k2shared", "pend_k2_fixedbw", "part_k2shared_fixedbw", "pend_k2_minbw", "part_k2_noisy_vel",
               "part_k2_fullcov"]


@pytest.mark.parametrize("name", K2_FIXTURES)
def test_restatement_vs_reference_goldens(golden, name):
    """Every (t, k) of every K2 fixture: phi_ref at bandwidth_ref against the reference's phi, fed the oracle's score() of the fixture's costs and
    actions (no fixture records the score), at k2_tolerance - the reference's own fp32 -2XY + XX + YY noise; bandwidth_ref against the
    bandwidths Oracle.phi_k2 returns at 1e-5 (test_seeded_vs_oracle's bound)."""
    g = golden(name)
    o = Oracle(**scenario_kwargs(g))
    T, K_ = g["eps"].shape[:2]
    shared = str(g["kernel_kind"]) == "K2shared"
    assert str(g["kernel_kind"]) in ("K2", "K2shared")
    fixed = float(g["k2_bandwidth"]) if "k2_bandwidth" in g else -1.0
    min_bw = float(g["k2_minimum_bw"]) if "k2_minimum_bw" in g else 1e-5
    theta = g["theta0"]
    for t in range(T):
        for k in range(K_):
            mu, mix = _prior_at(g, t, theta)
            _, _, sc = o.score(theta, mu, mix, _sig(g, "sigma_p"), g["costs"][t, k], g["actions"][t, k], float(g["alpha"]), _sig(g, "sigma_a"))
            h = K.bandwidth_ref(theta, shared, 1.0, fixed, min_bw)
            _, h_orc = o.phi_k2(theta, sc, indep=not shared, bandwidth=fixed, minimum_bw=min_bw)
            assert relerr(h, h_orc) < 1e-5, (name, t, k)
            phi = K.phi_ref(theta, sc, h, shared)
            assert elemerr(phi, g["phi"][t, k]) < k2_tolerance(theta, h, shared, int(g["da"])), (name, t, k)
            theta = g["theta_after"][t, k]
        theta = g["tick_theta_rolled"][t]


@pytest.mark.parametrize("indep", [True, False])
@pytest.mark.parametrize("N,da", [(64, 1), (64, 2), (300, 1), (300, 2)])
def test_restatement_vs_oracle(N, da, indep):
    """Beyond the fixtures' 6-16 particles: Oracle.phi_k2 (the reference's fp32 distance formula) at k2_tolerance, its bandwidths at 1e-5."""
    H = 3
    _, theta, score = K.inputs(N, H, da, seed=7 * N + da)
    o = Oracle(model="pendulum" if da == 1 else "particle", N=N, S=1, M=1, H=H)
    phi_orc, h_orc = o.phi_k2(theta, score, indep=indep)
    h = K.bandwidth_ref(theta, not indep)
    assert relerr(h, h_orc) < 1e-5
    assert elemerr(K.phi_ref(theta, score, h, not indep), phi_orc) < k2_tolerance(theta, h, not indep, da)


def test_bandwidth_ref_settings():
    """the clamp, the scale and the fixed-bandwidth rule (orc_phi_k2: double until the fp32 scalar) against the oracle"""
    N, H, da = 50, 3, 2
    _, theta, score = K.inputs(N, H, da, seed=5, ties=True)
    o = Oracle(model="particle", N=N, S=1, M=1, H=H)
    for indep in (True, False):
        for kw in (dict(bw_scale=0.5), dict(bandwidth=0.7), dict(bandwidth=0.7, bw_scale=0.5), dict(minimum_bw=0.8), dict(bandwidth=0.01, minimum_bw=0.3)):
            _, h_orc = o.phi_k2(theta, score, indep=indep, **kw)
            h = K.bandwidth_ref(theta, not indep, kw.get("bw_scale", 1.0), kw.get("bandwidth", -1.0), kw.get("minimum_bw", 1e-5))
            assert relerr(h, h_orc) < 1e-5, (indep, kw)
            if "bandwidth" in kw:
                assert np.array_equal(np.asarray(h, np.float32), h_orc)


@pytest.mark.parametrize("case", K.PHI_CASES + K.APPLY_CASES, ids=lambda c: c["id"])
def test_case_tolerance_and_power(case):
    """Per case of the GPU file, from the restatement alone: tol = max(1e-5, 2 d) <= 5e-5, every power variant >= 10 tol away.
    Measured: d = 1.2e-7 ... 3.5e-6 (0 with one or two particles; the table of DESIGN.md section 2), so every tolerance is the 1e-5 floor;
    the weakest variant is the last key left out at N = 3000, 9.4e-3."""
    d, tol, power = K.measure(case["id"])
    print("%s: d %.2e tol %.1e power %s" % (case["id"], d, tol, {v: "%.1e" % p for v, p in power.items()}))
    assert tol <= K.TOL_CAP, d
    assert power, "no power variant"
    for v, p in power.items():
        assert p >= 10 * tol, (v, p)


@pytest.mark.parametrize("case", [c for c in K.PHI_CASES if c["min_bw"] == "split"], ids=lambda c: c["id"])
def test_split_clamp_splits(case):
    _, theta, _ = K.case_inputs(case)
    h, m = K.case_bandwidths(case, theta), K.case_min_bw(case, theta)
    assert 1 <= int((h == m).sum()) <= h.size - 1
