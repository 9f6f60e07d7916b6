"""log p(theta) of SVMPC.forward on large sets whose prior means alias the particles, at every row width its kernels are compiled for,
against the float64 restatement of tests/logp_cases.py ("log p on large aliased sets at every compiled width").  The
independent side is plain numpy, pinned on the CPU by tests/test_logp_cases_cpu.py.  Every tolerance is logp_cases.measure(case): max(2e-6
(1 + |log p|max), 2 d_moved, 2 d) <= 2e-4 absolute on values of 15 - 73, with d measured from the restatements alone (never from device
output): d_prod of the float32 product form for the two product-form passes, d32 of the float32 exact-difference form for the third.

| implementation (dust_amd.hip launch_prior(logp_only)) | reached by | path on record |
| run-list pass: logp_prep_far_kernel<dpb>, far_lb_kernel<dpb>, far_flags_kernel<dpb, 64, true>, far_pack_kernel,
|   pairwise_logp_packed_kernel<dpb> | N >= 8192, default switches (tile order of query_order_kernel from the second pass 1 on);
|   DUST_PACK_ORDER=0 (index order); kernel = IMQ (pass 1 builds no tile order: qperm == nullptr behind a pass 1 of another path) |
|   dust_debug_far_logp: all == groups * chunks > 0; only N and the switches select the pass (no counter tells it from the next) |
| dense matrix-core pass with the pre-pass: logp_prep_far_kernel<dpb>, far_lb_kernel<dpb>, far_flags_kernel<dpb, 64, false>,
|   pairwise_logp_mfma_kernel<dpb> | N <= 2304 under DUST_PAIR_BIG=1, the FIRST log-p pass of a context | all == groups * chunks > 0 |
| ... without it: logp_prep_kernel<dpb>, pairwise_logp_mfma_kernel<dpb> | DUST_FAR=0 at every N; passes 2 - 16 behind a pre-pass that
|   found under 30 % far (logp_far_decide) | dust_debug_far_logp: (0, 0) |
| exact-difference pass: pairwise_logp_big_kernel<32 / 64 / 80> | DUST_LOGP_MFMA=0, N <= 2304 | only the switch selects it |

dpb = max(16, 16 ceil(D / 16)): D = 16, 17, 32, 33, 48, 49, 64, 65, 80 give 16, 32, 32, 48, 48, 64, 64, 80, 80.  Per case and mode a fresh
context (the switches are read at create): K1 (or IMQ), lr = 0, weighted_prior, the case's sigma_p; set_theta, set_prior(theta), set_a_mat,
svmpc_update_prior(mix); svmpc_optimize(state, 2) - the particles must come back bit for bit and the means alias them; ONE svmpc_forward();
log p from get_log_weights().  The reference is fed the mixture weights the context holds.  Each test asserts that every applicable wrong
variant of the restatement lies >= 10 tol away, that log p is finite exactly where the reference is, and the far-block counts: never more
far blocks than the float64 criterion of logp_cases.live_blocks allows where the groups are in index order, some on the islands and
clusters inputs, none on the dense cloud.
"""
import numpy as np
import pytest

import logp_cases as Q
from helpers import far_logp

pytestmark = pytest.mark.gpu
STATE = {"pendulum": [3.0, 0.0], "particle": [-9.0, -9.0, 0.0, 0.0]}
ALPHA = {"pendulum": 1e-2, "particle": 1e-4}
IMQ_ELL = 0.9
MODE_ENV = {"default": {}, "far0": {"DUST_FAR": "0"}, "order0": {"DUST_PACK_ORDER": "0"}, "mfma0": {"DUST_LOGP_MFMA": "0"}, "imq": {}}
RUNS = [(c, m) for c in Q.SMALL_CASES for m in ("default", "far0", "mfma0")]
RUNS += [(c, m) for c in Q.LARGE_CASES for m in ("default", "far0", "order0") + (("imq",) if c["imq"] else ())]


def _ctx(case, inp, kernel="K1"):
    from dust_amd import Context
    from oracle import grid_4x4_map  # data only (the demo's occupancy grid)

    model = case["model"]
    c = Context(model=model, N=case["N"], S=8, M=1, H=case["H"], kernel=kernel, imq_ell=IMQ_ELL, lr=0.0, alpha=ALPHA[model], sigma_a=0.5,
                sigma_p=inp["sigma_p"], weighted_prior=True, grid=grid_4x4_map() if model == "particle" else None, seed=case["seed"])
    c.set_theta(inp["theta"])
    c.set_prior(inp["theta"])
    c.set_a_mat(inp["theta"])
    c.svmpc_update_prior(inp["mix"])  # the means alias theta from here on
    return c


def _aliased(c, inp):
    """the particles as given, bit for bit, the prior means aliasing them; returns the mixture weights the context holds"""
    mu, mix = c.get_prior()
    assert np.array_equal(c.get_theta(), inp["theta"]), "lr = 0: the particles must stay"
    assert np.array_equal(mu, inp["theta"]), "the prior means must alias the particles"
    return mix


def _check(case, mode, lp, ref, tol):
    lp = np.asarray(lp, np.float64)
    assert np.array_equal(np.isfinite(lp), np.isfinite(ref)), "%s [%s]: log p is not finite where the reference is" % (case["id"], mode)
    err = float(np.abs(lp - ref).max())
    print("%s [dpb %d, %s]: log p err %.2e (tol %.2e)" % (case["id"], case["dpb"], mode, err, tol))
    assert err < tol, "%s [%s]: log p err %.3e, tol %.2e (worst row %d)" % (case["id"], mode, err, tol, int(np.abs(lp - ref).argmax()))


def _power(case, dist, tol):
    for v, p in dist.items():
        assert p >= 10 * tol, "%s: variant %s is only %.2e from the reference (10 tol = %.1e)" % (case["id"], v, p, 10 * tol)


@pytest.mark.parametrize("case,mode", RUNS, ids=lambda v: v["id"] if isinstance(v, dict) else v)
def test_large_set_logp_vs_float64(case, mode, monkeypatch):
    """One log-p pass per (case, mode) - the table of the module docstring."""
    if case["N"] <= Q.SMALL_N:
        monkeypatch.setenv("DUST_PAIR_BIG", "1")  # (N D <= 65536 runs the small-set launches by default)
    for k, v in MODE_ENV[mode].items():
        monkeypatch.setenv(k, v)
    m = Q.measure(case["id"])
    tol = m["tol_exact"] if mode == "mfma0" else m["tol"]
    assert tol <= Q.TOL_CAP
    _power(case, {v: m["power"][v] for v in Q.logp_variants(case)}, tol)
    inp = Q.case_inputs(case)
    c = _ctx(case, inp, "IMQ" if mode == "imq" else "K1")
    c.svmpc_optimize(np.array(STATE[case["model"]], np.float32), 2)
    mix = _aliased(c, inp)
    c.svmpc_forward()
    far, units = far_logp(c)
    _, lp = c.get_log_weights()
    c.close()
    _check(case, mode, lp, Q.reference(case, mix), tol)
    if mode == "mfma0":  # (the exact-difference pass has no pre-pass)
        return
    if mode == "far0":
        assert (far, units) == (0, 0), (far, units)
        return
    groups = (case["N"] + 63) // 64
    may = int((~m["live"]).sum())
    print("%s [%s]: %d of %d blocks far (float64 criterion: %d)" % (case["id"], mode, far, units, may))
    assert units == groups * groups > 0, (units, groups)
    run_list = case["N"] >= 8192
    if not run_list or mode in ("order0", "imq"):  # groups in index order: the device may never drop a block the float64 criterion calls live
        assert far <= may, (far, may)
    if case["family"] == "dense":
        assert far == 0, far
    else:
        assert far > 0


def test_logp_prepass_decision(monkeypatch):
    """logp_far_decide (dust_amd.hip, the comment above far_counts_alloc) on a dense cloud at N = 2304, far share 0: the first log-p pass
    of a context runs the pre-pass; one that found under 30 % far is followed by 15 passes without one (bit-identical to each other and
    to a DUST_FAR=0 context), then probed again.  The particles and weights are put back before every forward (forward rolls the
    particles and, with weighted_prior, refreshes the weights).  Every one of the 17 log p arrays within tol."""
    monkeypatch.setenv("DUST_PAIR_BIG", "1")
    case = Q.case_by_id(Q.DECIDE_CASE_ID)
    m = Q.measure(case["id"])
    assert m["far_share"] == 0.0 and m["tol"] <= Q.TOL_CAP
    inp = Q.case_inputs(case)
    state = np.array(STATE[case["model"]], np.float32)

    def forwards(n):
        c = _ctx(case, inp)
        c.svmpc_optimize(state, 2)
        out = []
        for _ in range(n):
            c.set_theta(inp["theta"])
            c.svmpc_update_prior(inp["mix"])
            mix = _aliased(c, inp)
            c.svmpc_forward()
            out.append((far_logp(c), c.get_log_weights()[1], mix))
        c.close()
        return out

    got = forwards(17)
    monkeypatch.setenv("DUST_FAR", "0")
    ((far0, lp0, _),) = forwards(1)
    assert far0 == (0, 0)
    groups = (case["N"] + 63) // 64
    counts = [g[0] for g in got]
    print("far-block reports of 17 forwards:", counts)
    for k in (0, 16):
        assert counts[k] == (0, groups * groups), (k + 1, counts)
    assert counts[1:16] == [(0, 0)] * 15, counts
    for k, (_, lp, mix) in enumerate(got):
        _check(case, "forward %d" % (k + 1), lp, Q.reference(case, mix), m["tol"])
    for _, lp, _ in got[1:16]:
        assert np.array_equal(lp, got[1][1]) and np.array_equal(lp, lp0)
