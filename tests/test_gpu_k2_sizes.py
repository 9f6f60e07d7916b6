"""Every K2 Stein kernel of dust_amd/csrc/bandwidth.hpp against a float64 restatement at multi-tile sizes ("K2 beyond
the fixtures").  The independent side is tests/k2_cases.py - plain float64 numpy with exact differences, pinned on the CPU by
tests/test_k2_cases_cpu.py - evaluated STAGE-WISE: phi is compared at the device's own score and its own bandwidths, the bandwidths are held
separately.  Every phi tolerance is k2_cases.tolerance(case) = max(1e-5, 2 d) <= 5e-5 with d measured from the restatement alone (never from
device output); the bandwidth bound is the derived 1e-6 (below).  Sizes are the smallest that reach a code path of `launch_k2_phi`:

| kernel | contexts | N |
| k2_phi3_kernel (N <= 2048: 16 key slices of (N + 15) >> 4, 128 queries per workgroup) | K2 on Pendulum (d_a = 1); K2 on Particle (d_a = 2,
|   D = 2 H); K2shared on Pendulum (G = H) | 1, 2, 15, 17 (slices without keys), 127, 128, 129 (query tile edge), 1000, 2047, 2048 |
| k2_phi2_kernel (N > 2048: 2048-key chunks through LDS, 4 slices) | K2 on Pendulum; 2049 on Particle too | 2049 (a chunk of one key), 3000,
|   4097 (three chunks) |
| k2_phi_kernel<2> (K2shared on Particle: 64 queries per workgroup, 2048-key chunks, 4 slices) | | 1, 2, 3, 63, 64, 65 (second tile with one
|   query), 300, 2048, 2049, 2100 (second chunk, ragged tile) |
H = 3 (H = 2 for d_a = 2 beyond N = 2048), S = 8.  No size was refused by another part of the library.
"""
import numpy as np
import pytest

import k2_cases as K
from helpers import elemerr

pytestmark = pytest.mark.gpu
S = 8
STATE = {"pendulum": [3.0, 0.0], "particle": [-5.2, -7.3, 4.0, 3.0]}
SIGMA = {"pendulum": 2.0, "particle": 5.0}
ALPHA = {"pendulum": 1.0, "particle": 1e-4}
LR = 0.5
# |h_dev - bandwidth_ref| <= BW_TOL bandwidth_ref: every fp32 pair distance is within 4 * 2^-24 relative of its float64 value (the differences
# are exact to 2^-24 each, squared, one fp32 sum), an order statistic moves by no more than its entries, the division by log(N + 1) and the
# scale add 2 * 2^-24: 3.6e-7; the rest is margin for the reference's own log.  At N <= 65 neighbouring order statistics are far apart, so
# the bound also pins the rank.
BW_TOL = 1e-6


def _ctx(case, theta, mu, **kw):
    from dust_amd import Context
    from oracle import grid_4x4_map  # data only (the demo's occupancy grid)

    model = case["model"]
    kw = dict(dict(model=model, N=case["N"], S=S, M=1, H=case["H"], kernel=case["kernel"], lr=LR, alpha=ALPHA[model], sigma_a=SIGMA[model],
                   sigma_p=SIGMA[model], bw_scale=case["bw_scale"]), **kw)
    if case["fixed_bw"] >= 0:
        kw["k2_bandwidth"] = case["fixed_bw"]
    if case["min_bw"] != 1e-5:
        kw["k2_minimum_bw"] = K.case_min_bw(case, theta)
    c = Context(grid=grid_4x4_map() if model == "particle" else None, **kw)
    c.set_theta(theta)
    c.set_prior(mu)
    c.set_a_mat(theta)
    return c


def _costs_actions(case, theta):
    """small S, costs and actions from numpy: softmax(-alpha costs) spreads over the samples, the actions scatter around the particles"""
    rng = np.random.default_rng(case["seed"] + 2)
    model = case["model"]
    eps = rng.standard_normal((S,) + theta.shape).astype(np.float32)
    actions = (theta[None] + np.float32(SIGMA[model]) * eps).astype(np.float32)
    costs = rng.uniform(0.0, 3.0 / ALPHA[model], (S, case["N"])).astype(np.float32)
    return costs, actions


def _bw_ok(h_dev, ref):
    ref = np.asarray(ref, np.float64)
    return bool(np.all(np.abs(np.asarray(h_dev, np.float64) - ref) <= BW_TOL * ref))


@pytest.mark.parametrize("case", K.PHI_CASES, ids=lambda c: c["id"])
def test_phi_vs_float64_restatement(case):
    """phi of `case["dev"]` (the module's table) at the device's own score and bandwidths against phi_ref; the settings cases at N = 300 carry
    a fixed bandwidth (0.7), a clamp that splits the groups (asserted) and a bandwidth scale of 0.5.  The bandwidths themselves are held to
    bandwidth_ref at the derived bound (fixed: the fp32 value exactly)."""
    tol = K.tolerance(case)
    shared = case["kernel"] == "K2shared"
    mu, theta, _ = K.case_inputs(case)
    c = _ctx(case, theta, mu)
    costs, actions = _costs_actions(case, theta)
    phi, _, _ = c.svmpc_phi(costs, actions)
    score, h = c.get_score(), c.get_bandwidths()
    c.close()
    assert np.isfinite(score).all() and float(np.abs(score).max()) > 0
    h_ref = K.case_bandwidths(case, theta)
    if case["fixed_bw"] >= 0:
        assert np.array_equal(h, h_ref)
    else:
        assert _bw_ok(h, h_ref), (h, h_ref)
    if case["min_bw"] == "split":
        assert 1 <= int((h == np.float32(K.case_min_bw(case, theta))).sum()) <= h.size - 1
    err = elemerr(phi, K.phi_ref(theta, score, h, shared))
    print("%s: phi err %.2e (tol %.1e)" % (case["id"], err, tol))
    assert err < tol


@pytest.mark.parametrize("N", K.BW_SHARED_N)
def test_shared_bandwidths_vs_float64_order_statistic(N):
    """k2_bandwidth_pairs_kernel (K2shared on Particle) at the sizes of its phi row, with ties (the first N // 7 particles share timestep 1)
    and a constant column: within BW_TOL of the float64 lower-middle order statistic; at N = 1 and 2 that entry is a zero distance and the
    result is exactly the clamp.  Once more after set_theta of nudged particles."""
    case = next(c for c in K.PHI_CASES if c["id"] == "phiS-part-K2shared-%d" % N)
    mu, theta, _ = K.case_inputs(case, ties=True)
    c = _ctx(case, theta, mu)
    costs, actions = _costs_actions(case, theta)
    for nudge in (None, 1.002):
        if nudge is not None:
            theta = (theta * np.float32(nudge)).astype(np.float32)
            c.set_theta(theta)
        c.svmpc_phi(costs, actions)
        h, ref = c.get_bandwidths(), K.bandwidth_ref(theta, True)
        print("N %d%s: bandwidth err %.2e" % (N, "" if nudge is None else " nudged", float((np.abs(h - ref) / ref).max())))
        assert _bw_ok(h, ref), (nudge, h, ref)
        if N <= 2:
            assert np.all(h == np.float32(1e-5))
        else:
            assert np.all(h > np.float32(1e-5))
    c.close()


@pytest.mark.parametrize("case", K.APPLY_CASES, ids=lambda c: c["id"])
def test_step_inside_the_phi_kernel(case):
    """The optimiser step riding in the phi kernel (`apply`, `thetaT_out`, `k2_thetaT_fresh`): contexts A and B from the same inputs, SGD,
    caller-supplied eps.  B takes one iteration: its particles are fmaf(lr, phi, theta0) bit for bit.  A takes two in one call: its second
    iteration reads the TRANSPOSED copy the first one wrote - its bandwidths are those of B's particles, its phi is phi_ref at B's
    particles (A's own score and bandwidths), its particles are fmaf(lr, phi, theta_B) exactly."""
    from oracle import Oracle

    tol = K.tolerance(case)
    shared = case["kernel"] == "K2shared"
    mu, theta0, _ = K.case_inputs(case)
    eps = np.random.default_rng(case["seed"] + 3).standard_normal((2, S) + theta0.shape).astype(np.float32)
    state = np.array(STATE[case["model"]], np.float32)
    a, b = _ctx(case, theta0, mu), _ctx(case, theta0, mu)
    b.svmpc_optimize(state, 1, eps[:1])
    phi_b, theta_b = b.get_phi(), b.get_theta()
    b.close()
    assert float(np.abs(phi_b).max()) > 0
    assert np.array_equal(theta_b, Oracle.sgd(theta0, phi_b, LR))
    a.svmpc_optimize(state, 2, eps[:2])
    phi_a, theta_a, score_a, h_a = a.get_phi(), a.get_theta(), a.get_score(), a.get_bandwidths()
    a.close()
    assert _bw_ok(h_a, K.bandwidth_ref(theta_b, shared)), h_a
    err = elemerr(phi_a, K.phi_ref(theta_b, score_a, h_a, shared))
    print("%s: second-iteration phi err %.2e (tol %.1e)" % (case["id"], err, tol))
    assert err < tol
    assert np.array_equal(theta_a, Oracle.sgd(theta_b, phi_a, LR))


@pytest.mark.parametrize("model,N", [("pendulum", 1), ("pendulum", 2), ("particle", 2), ("pendulum", 3)])
def test_fewest_particles_through_the_loop(model, N):
    """The per-dimension bandwidths of K2 inside the optimisation loop (`k2_bandwidth256` as a role of the prior + rollout launch where that
    launch takes the shape, `k2_bandwidth_sorted_kernel` otherwise).  With two particles the lower-middle of the four distances is one of
    the diagonal's zeros: no pair is wanted, the bandwidth is the clamp.  Both selections kept a bracket whose invariant needs a wanted
    pair and read the answer from lane -1 of the candidate sort: +inf (found by test_phi_vs_float64_restatement at N = 2)."""
    case = next(c for c in K.PHI_CASES if c["id"] == "phi3-%s-K2-%d" % (model[:4], min(N, 2)))
    case = dict(case, N=N, seed=case["seed"] + N)
    mu, theta, _ = K.case_inputs(case)
    eps = np.random.default_rng(N).standard_normal((1, S) + theta.shape).astype(np.float32)
    c = _ctx(case, theta, mu)
    c.svmpc_optimize(np.array(STATE[model], np.float32), 1, eps)
    h, phi, th = c.get_bandwidths(), c.get_phi(), c.get_theta()
    c.close()
    assert _bw_ok(h, K.bandwidth_ref(theta, False)), h
    if N <= 2:
        assert np.all(h == np.float32(1e-5))
    assert np.isfinite(phi).all() and np.isfinite(th).all()


def test_shared_median_pass_refuses_what_its_lds_cannot_hold():
    """k2_bandwidth_pairs_kernel keeps the d_a * N coordinates of a group in dynamic LDS and nobody raises the function's limit: above 64 KB
    (d_a = 2: N = 8193) `launch_k2_bandwidth` refuses the shape on the host (DUST_ERR_UNSUPPORTED) instead of a failed launch.  A fixed
    bandwidth needs no median pass: the same shape runs."""
    from dust_amd import _lib as L

    case = dict(K.PHI_CASES[0], model="particle", kernel="K2shared", N=8193, H=1, da=2, seed=8193)
    mu, theta, _ = K.case_inputs(case)
    costs, actions = _costs_actions(case, theta)
    c = _ctx(case, theta, mu)
    with pytest.raises(L.DustError) as e:
        c.svmpc_phi(costs, actions)
    assert e.value.status == L.ERR_UNSUPPORTED
    c.close()
    c = _ctx(dict(case, fixed_bw=0.7), theta, mu)
    phi, _, _ = c.svmpc_phi(costs, actions)
    assert np.isfinite(phi).all() and np.array_equal(c.get_bandwidths(), K.bandwidth_ref(theta, True, fixed_bw=0.7))
    c.close()
