"""The K2 Stein step beyond the 8-particle fixtures (TEST INFRASTRUCTURE): a float64 numpy restatement of iid_mp(RBF)
(svmpc.py:64-74 -> composite_kernels.py:33-64 -> base_kernels.py:53-108) with EXACT differences, the seeded inputs and the case table
shared by tests/test_k2_cases_cpu.py (which pins the restatement and measures every tolerance from it alone) and
tests/test_gpu_k2_sizes.py (which holds the kernels of dust_amd/csrc/bandwidth.hpp to it).  Numpy only: nothing here imports the
reference, the oracle or the library.

Why not the oracle: `orc_phi_k2` follows the reference's fp32 `-2XY + XX + YY` distances, whose cancellation noise grows with x^2 / h
(helpers.k2_tolerance), and sorts N^2 floats per dimension.  The restatement is evaluated STAGE BY STAGE: the
bandwidths are one stage (`bandwidth_ref`), phi at GIVEN bandwidths and a GIVEN score another (`phi_ref`) - the device's own score and
its own bandwidths are fed into the phi reference, the bandwidths are held separately.

A case is a dict: id, model, kernel ("K2": one kernel per scalar dimension; "K2shared": one per timestep over the d_a controls), N, H, da,
seed, spread (None: column scales cycling through COLUMN_SCALES; a number: that scale for every column), bw_scale, fixed_bw (< 0: the
median trick), min_bw (a number, or "split": chosen from bandwidth_ref so that some groups are clamped and some are free), dev (the phi
kernel `launch_k2_phi` picks for the shape).
"""
import functools

import numpy as np

from helpers import elemerr

COLUMN_SCALES = (1.0, 2.0, 0.5)
VARIANTS = ("drop_last", "one_over_h", "rot_h", "per_dim")
TOL_FLOOR, TOL_CAP = 1e-5, 5e-5


def inputs(N, H, da, seed, spread=None, ties=False):
    """(mu, theta, score), all fp32 [N, H, da]: mu ~ N(0, 1), theta = mu + column_scale N(0, 1) with the scales cycling over the H * da
    columns (neighbouring groups get visibly different bandwidths), score = 2 N(0, 1).  ties: the bandwidth cases - the first N // 7
    particles share timestep 1 (ties and zero distances) and one column is constant, as test_k2_bandwidth_is_the_exact_order_statistic
    has them."""
    rng = np.random.default_rng(seed)
    D = H * da
    mu = rng.standard_normal((N, H, da)).astype(np.float32)
    sc = np.array([COLUMN_SCALES[c % 3] for c in range(D)] if spread is None else [spread] * D, np.float32).reshape(1, H, da)
    theta = (mu + sc * rng.standard_normal((N, H, da)).astype(np.float32)).astype(np.float32)
    score = (2.0 * rng.standard_normal((N, H, da))).astype(np.float32)
    if ties:
        theta[: N // 7, 1] = theta[0, 1]
        theta[:, H - 1, 0] = 1.25
    return mu, theta, score


def _groups(H, da, shared):
    gd = da if shared else 1
    return (H if shared else H * da), gd


def phi_ref(theta, score, h, shared, dtype=np.float64, variant=None, block=256):
    """phi [N, H, da] in `dtype`.  Per kernel group g (one dimension, or the da dimensions of a timestep when shared):
    df = x_i - x_j, d2 = sum_q df_q^2, k = exp(-d2 / h_g), phi_ic = (sum_j k s_jc) / N + ((sum_j k df_c) 2 / h_g) / N.
    variant (power): "drop_last" the last key left out, "one_over_h" the repulsion factor 1 / h, "rot_h" the bandwidths rotated by one
    group, "per_dim" (shared) per-dimension distances instead of the joint one."""
    theta = np.asarray(theta)
    N, H, da = theta.shape
    G, gd = _groups(H, da, shared)
    x = theta.reshape(N, H * da).astype(dtype)
    s = np.asarray(score).reshape(N, H * da).astype(dtype)
    h = np.asarray(h, dtype).reshape(G)
    if variant == "rot_h":
        h = np.roll(h, 1)
    nk = N - 1 if variant == "drop_last" else N
    rep = dtype(1.0 if variant == "one_over_h" else 2.0)
    n = dtype(N)
    out = np.zeros((N, H * da), dtype)
    for g in range(G):
        c = slice(g * gd, (g + 1) * gd)
        xk, sk = x[:nk, c], s[:nk, c]
        for i0 in range(0, N, block):
            df = x[i0:i0 + block, None, c] - xk[None, :, :]  # [B, nk, gd]
            if variant == "per_dim":
                k = np.exp(-(df * df) / h[g])
                a, r = (k * sk[None]).sum(1), (k * df).sum(1)
            else:
                k = np.exp(-(df * df).sum(-1) / h[g])  # [B, nk]
                a, r = k @ sk, np.einsum("ij,ijq->iq", k, df)
            out[i0:i0 + block, c] = a / n + (r * rep / h[g]) / n
    return out.reshape(N, H, da)


def bandwidth_ref(theta, shared, bw_scale=1.0, fixed_bw=-1.0, min_bw=1e-5):
    """The bandwidths [G].  Median trick (fixed_bw < 0): the lower-middle order statistic, index (N^2 - 1) // 2, of all N^2 float64 squared
    distances of the group, over log(N + 1), times bw_scale, clamped at min_bw (float64).  Fixed bandwidth: bw_scale fixed_bw^2 / log(N + 1)
    in double, then the clamp, then fp32 (base_kernels.py:66-67 keeps Python floats until the tensor ops)."""
    theta = np.asarray(theta)
    N, H, da = theta.shape
    G, gd = _groups(H, da, shared)
    bw_scale, fixed_bw, min_bw = (float(np.float32(v)) for v in (bw_scale, fixed_bw, min_bw))  # (the three settings are fp32 numbers)
    if fixed_bw >= 0:
        hd = fixed_bw * fixed_bw
        hd = hd / np.log(N + 1.0)
        hd = bw_scale * hd
        return np.full(G, np.float32(max(hd, min_bw)), np.float32)
    x = theta.reshape(N, H * da).astype(np.float64)
    r = (N * N - 1) // 2
    out = np.empty(G, np.float64)
    for g in range(G):
        d2 = np.zeros((N, N), np.float64)
        for q in range(g * gd, (g + 1) * gd):
            df = x[:, None, q] - x[None, :, q]
            d2 += df * df
        med = np.partition(d2.reshape(-1), r)[r]
        out[g] = max(bw_scale * (med / np.log(N + 1.0)), min_bw)
    return out


def ulp_moved(theta, seed):
    """theta with every entry moved one fp32 ulp in a seeded random direction"""
    up = np.random.default_rng(seed).integers(0, 2, theta.shape).astype(bool)
    return np.where(up, np.nextafter(theta, np.float32(np.inf)), np.nextafter(theta, np.float32(-np.inf))).astype(np.float32)


# ---- the case table ("K2 beyond the fixtures")
def _case(tag, model, kernel, N, dev, H=None, spread=None, bw_scale=1.0, fixed_bw=-1.0, min_bw=1e-5):
    da = 1 if model == "pendulum" else 2
    if H is None:
        H = 2 if (da == 2 and N > 2048) else 3
    cid = "%s-%s-%s-%d" % (tag, model[:4], kernel, N)
    return dict(id=cid, model=model, kernel=kernel, N=N, H=H, da=da, seed=1000 + N, spread=spread, bw_scale=bw_scale, fixed_bw=fixed_bw,
                min_bw=min_bw, dev=dev)


PHI3_N = (1, 2, 15, 17, 127, 128, 129, 1000, 2047, 2048)  # slices without keys, the 128-query tile edge, the last size of the kernel
PHI2_N = (2049, 3000, 4097)                                # a chunk of one key, two ragged chunks, three chunks
PHI_SHARED_N = (1, 2, 3, 63, 64, 65, 300, 2048, 2049, 2100)  # 64-query tile edge, second chunk of one key, second chunk + ragged tile

PHI_CASES = []
for _n in PHI3_N:
    PHI_CASES += [_case("phi3", "pendulum", "K2", _n, "k2_phi3_kernel"), _case("phi3", "particle", "K2", _n, "k2_phi3_kernel"),
                  _case("phi3", "pendulum", "K2shared", _n, "k2_phi3_kernel")]
for _n in PHI2_N:
    PHI_CASES.append(_case("phi2", "pendulum", "K2", _n, "k2_phi2_kernel"))
PHI_CASES.append(_case("phi2", "particle", "K2", 2049, "k2_phi2_kernel"))
PHI_CASES.append(_case("phi2-spread", "pendulum", "K2", 3000, "k2_phi2_kernel", spread=0.3))
for _n in PHI_SHARED_N:
    PHI_CASES.append(_case("phiS", "particle", "K2shared", _n, "k2_phi_kernel<2>"))
PHI_CASES.append(_case("phiS-spread", "particle", "K2shared", 300, "k2_phi_kernel<2>", spread=0.3))
# settings at N = 300, for both kernels: a fixed bandwidth, a clamp that splits the groups, a non-unit bandwidth scale
for _model, _kernel, _dev in (("pendulum", "K2", "k2_phi3_kernel"), ("particle", "K2shared", "k2_phi_kernel<2>")):
    PHI_CASES += [_case("fixed", _model, _kernel, 300, _dev, fixed_bw=0.7), _case("minbw", _model, _kernel, 300, _dev, min_bw="split"),
                  _case("scale", _model, _kernel, 300, _dev, bw_scale=0.5)]
del _n, _model, _kernel, _dev

BW_SHARED_N = PHI_SHARED_N  # k2_bandwidth_pairs_kernel: the same N as its phi row, with ties and the constant column
APPLY_CASES = [_case("apply", "particle", "K2shared", 65, "k2_phi_kernel<2>"), _case("apply", "particle", "K2shared", 2049, "k2_phi_kernel<2>"),
               _case("apply", "pendulum", "K2", 2049, "k2_phi2_kernel")]


def case_inputs(case, ties=False):
    return inputs(case["N"], case["H"], case["da"], case["seed"], case["spread"], ties=ties)


def case_min_bw(case, theta):
    """The clamp of a case.  "split": the geometric mean of the two middle free bandwidths - at least one group clamped, one free."""
    if case["min_bw"] != "split":
        return float(case["min_bw"])
    h = np.sort(bandwidth_ref(theta, case["kernel"] == "K2shared", case["bw_scale"]))
    m = h.size // 2
    return float(np.float32(np.sqrt(h[m - 1] * h[m])))


def case_bandwidths(case, theta):
    return bandwidth_ref(theta, case["kernel"] == "K2shared", case["bw_scale"], case["fixed_bw"], case_min_bw(case, theta))


def case_variants(case):
    """The power variants that can show at a case's shape.  With one or two particles the lower-middle distance is a zero, every bandwidth
    is the clamp (1e-5) and the kernel value of the one distinct pair underflows to 0: phi_i = s_i / N whatever h is, so only the variant
    that drops a KEY differs.  per_dim needs a joint distance, rot_h bandwidths that differ (not one fixed value)."""
    if case["N"] <= 2:
        return ("drop_last",)
    out = tuple(v for v in VARIANTS if v != "per_dim" or (case["kernel"] == "K2shared" and case["da"] > 1))
    return tuple(v for v in out if v != "rot_h" or case["fixed_bw"] < 0)


def _case_by_id(cid):
    for c in PHI_CASES + APPLY_CASES:
        if c["id"] == cid:
            return c
    raise KeyError(cid)


@functools.lru_cache(maxsize=None)
def measure(cid):
    """(d, tol, {variant: distance}) of a case, from the restatement alone (the project's rule):
    d = max(elemerr(phi_ref(theta moved one fp32 ulp per entry), phi_ref(theta)), elemerr(phi_ref(dtype=float32), phi_ref(theta))) at
    fixed h; tol = max(1e-5, 2 d).  Never computed from device output."""
    case = _case_by_id(cid)
    shared = case["kernel"] == "K2shared"
    _, theta, score = case_inputs(case)
    h = case_bandwidths(case, theta)
    ref = phi_ref(theta, score, h, shared)
    d = max(elemerr(phi_ref(ulp_moved(theta, case["seed"] + 1), score, h, shared), ref),
            elemerr(phi_ref(theta, score, h, shared, dtype=np.float32), ref))
    power = {v: elemerr(phi_ref(theta, score, h, shared, variant=v), ref) for v in case_variants(case)}
    return d, max(TOL_FLOOR, 2.0 * d), power


def tolerance(case):
    d, tol, _ = measure(case["id"])
    assert tol <= TOL_CAP, (case["id"], d)
    return tol
