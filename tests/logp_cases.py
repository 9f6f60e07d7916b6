"""log p(theta) of SVMPC.forward on LARGE sets whose prior means alias the particles (TEST INFRASTRUCTURE): a float64 numpy restatement in
the centred product form, the float64 far-block criterion, seeded "islands" inputs whose (64-query group, 64-key chunk) blocks are partly
far and partly near, and the case table shared by tests/test_logp_cases_cpu.py (which pins the restatement against the exact-difference
prior_ref and measures every tolerance from the restatements alone) and tests/test_gpu_logp_sizes.py (which holds the three log-p passes of
dust_amd.hip launch_prior(logp_only) - the run-list pass, the dense matrix-core pass, the exact-difference pass - to it at every compiled
row width).  Numpy only: nothing here imports the reference, the oracle or the library.  The sibling of tests/pairwise_cases.py.

Why a second restatement: prior_ref forms exact differences, [b, N, D] of them - 16-20 s at N = 8192.  The product form
q_ij = |z_i|^2 + |z_j|^2 - 2 z_i . z_j on rows centred on particle 0 is one matrix product (1.4 s at N = 8192, 5 s at 16384) and in float64
its cancellation is ~1e-13 on these inputs (pinned at 1e-10 against prior_ref by the CPU module).  The same form in float32 IS the device's
form (pairwise_logp_mfma.hpp), so `dtype=np.float32` measures what the form costs there.

A case is a dict: id, model, N, H, da, D, dpb (the padded row width the kernels are compiled for: max(16, 16 ceil(D / 16))), family
("islands", "dense": the cloud of pairwise_cases, no far block; "clusters": two dense halves 150 scaled units apart), weights ("flat" rand +
0.05; "steep" exp(-6 u); "zeros" exact zeros over keys 0 ... 63 and a scattered tenth), seed.
"""
import functools

import numpy as np

from pairwise_cases import _keys, cloud, log_mix, log_norm, prior_ref, ulp_moved

LN2 = float(np.log(2.0))
LOGP_VARIANTS = ("drop_last", "drop_chunk", "uniform_mix", "swap_sigma")
TOL_CAP = 2e-4  # the product form's own error must never turn a test vacuous
FAR_NATS = 30.0  # T / 2 of DUST_FAR_T_DEFAULT (pairwise_far.hpp): a skipped term is below e^-30 of its query's leading term
SMALL_N = 2304  # up to here the exact-difference restatement (and the exact-difference device pass) is part of a case


def _scaled(theta, sigma_p, dtype, swap=False):
    """z = (x - x_0) / sigma [N, D] in `dtype` (swap: the two scales exchanged)"""
    theta = np.asarray(theta)
    N, da = theta.shape[0], theta.shape[-1]
    x = theta.reshape(N, -1).astype(dtype)
    sg = np.broadcast_to(np.asarray(sigma_p, np.float32).reshape(-1), (da,)).astype(dtype)
    if swap:
        sg = sg[::-1]
    return (x - x[0:1]) / np.tile(sg, x.shape[1] // da)[None, :]


def _rows_per_block(N):
    """about 1024 query rows, whole 64-query groups, at most 2^23 logits per block"""
    return max(64, min(1024, ((1 << 23) // max(1, N)) // 64 * 64))


def _lse(lg):
    m = lg.max(1)
    return m + np.log(np.exp(lg - m[:, None]).sum(1))


def logp_all(theta, mix, sigma_p, dtype=np.float64, variants=(), live_nats=None):
    """({None: log p [N], variant: ...}, live or None): log p of the mixture sum_j pi_j N(x_i; x_j, diag sigma^2) WITHOUT its constant
    (`log_norm`), in the centred product form: z = (x - x_0) / sigma, q_ij = |z_i|^2 + |z_j|^2 - 2 z_i . z_j with q_ii = 0 put in exactly,
    logits_ij = log_mix(mix)_j - q_ij / 2, max-shifted log-sum-exp over j, in row blocks.  Every operation in `dtype`.  Variants:
    "drop_last" / "drop_chunk" keys left out (the last; 64 ... 127), "uniform_mix" the weights ignored, "swap_sigma" the two scales
    exchanged.  live_nats (float64 only): also the [groups, chunks] bool array of `live_blocks`, from the same logits."""
    theta = np.asarray(theta)
    N = theta.shape[0]
    z = _scaled(theta, sigma_p, dtype)
    n = (z * z).sum(1)
    lm = log_mix(mix, dtype)
    half, two = dtype(0.5), dtype(2.0)
    out = {v: np.empty(N, dtype) for v in (None,) + tuple(variants)}
    gone = {v: np.setdiff1d(np.arange(N), _keys(N, v)) for v in variants if v in ("drop_last", "drop_chunk")}
    if "swap_sigma" in variants:
        zs = _scaled(theta, sigma_p, dtype, swap=True)
        ns = (zs * zs).sum(1)
    groups, chunks = (N + 63) // 64, (N + 63) // 64
    live = np.zeros((groups, chunks), bool) if live_nats is not None else None
    B = _rows_per_block(N)
    for i0 in range(0, N, B):
        i1 = min(i0 + B, N)
        b, own = i1 - i0, (np.arange(i1 - i0), np.arange(i0, i1))
        q = (n[i0:i1, None] + n[None, :]) - two * (z[i0:i1] @ z.T)
        q[own] = dtype(0.0)
        lg = lm[None, :] - half * q
        m = lg.max(1)
        e = np.exp(lg - m[:, None])
        zsum = e.sum(1)
        out[None][i0:i1] = m + np.log(zsum)
        if live is not None:
            gb = (b + 63) // 64
            near = np.zeros((gb * 64, chunks * 64), bool)
            near[:b, :N] = lg >= (m - dtype(live_nats))[:, None]
            live[i0 // 64: i0 // 64 + gb] = near.reshape(gb, 64, chunks, 64).any(axis=(1, 3))
        for v in variants:
            if v in gone:
                # the same sum without the dropped keys: by subtraction where they carry under 1e-6 of it, from the logits elsewhere
                eg = e[:, gone[v]].sum(1)
                res = m + np.log(np.maximum(zsum - eg, dtype(1e-30)))
                rows = np.flatnonzero(eg > dtype(1e-6) * zsum)
                if len(rows):
                    res[rows] = _lse(np.delete(lg[rows], gone[v], axis=1))
                out[v][i0:i1] = res
            elif v == "uniform_mix":
                out[v][i0:i1] = _lse(-np.log(dtype(N)) - half * q)
            elif v == "swap_sigma":
                qs = (ns[i0:i1, None] + ns[None, :]) - two * (zs[i0:i1] @ zs.T)
                qs[own] = dtype(0.0)
                out[v][i0:i1] = _lse(lm[None, :] - half * qs)
            else:
                raise KeyError(v)
    return out, live


def logp_ref(theta, mix, sigma_p, dtype=np.float64, variant=None):
    return logp_all(theta, mix, sigma_p, dtype, () if variant is None else (variant,))[0][variant]


def live_blocks(theta, mix, sigma_p, nats=FAR_NATS):
    """[groups, chunks] bool, 64-query groups in index order against 64-key chunks (float64): True where SOME term of the block lies within
    `nats` of its own query's largest logit.  A block the device may call far must be False here: the device's bound is a lower bound on
    the distance and its reference m0 is at most the true maximum (pairwise_far.hpp)."""
    return logp_all(theta, mix, sigma_p, live_nats=nats)[1]


def live_blocks_brute(theta, mix, sigma_p, nats=FAR_NATS):
    """the same from exact differences, pair by pair (the CPU module holds `live_blocks` to it at one small case)"""
    theta = np.asarray(theta)
    N, da = theta.shape[0], theta.shape[-1]
    x = theta.reshape(N, -1).astype(np.float64)
    sg = np.tile(np.broadcast_to(np.asarray(sigma_p, np.float32).reshape(-1), (da,)).astype(np.float64), x.shape[1] // da)
    lm = log_mix(mix)
    nb = (N + 63) // 64
    live = np.zeros((nb, nb), bool)
    for i in range(N):
        d = (x - x[i]) / sg
        lg = lm - 0.5 * (d * d).sum(1)
        near = np.flatnonzero(lg >= lg.max() - nats)
        live[i // 64, np.unique(near // 64)] = True
    return live


# ---- seeded inputs
def islands(rng, N, H, da, sigma_p):
    """theta [N, H, da] fp32: index runs of 17 - 200 particles (not aligned to 64), one island each.  Island centres N(0, 1) sigma sqrt(150 /
    (2 D)) per coordinate (squared scaled distance between two: ~150); every fourth island instead sqrt(60 / D) sigma per coordinate (in a
    random direction) from its predecessor - squared scaled distance 60, its pair terms straddle the 30-nat threshold; width ln2 / sqrt(D)
    inside an island; a tenth of the particles re-assigned to random islands, so most blocks are partly near."""
    D = H * da
    sg = np.tile(np.broadcast_to(np.asarray(sigma_p, np.float64).reshape(-1), (da,)), H)
    runs = []
    while sum(runs) < N:
        runs.append(int(rng.integers(17, 201)))
    runs[-1] -= sum(runs) - N
    K = len(runs)
    centres = np.empty((K, D))
    for k in range(K):
        if k % 4 == 3:
            centres[k] = centres[k - 1] + np.sqrt(60.0 / D) * sg * rng.choice([-1.0, 1.0], D)
        else:
            centres[k] = rng.standard_normal(D) * sg * np.sqrt(150.0 / (2.0 * D))
    isl = np.repeat(np.arange(K), runs)
    moved = rng.permutation(N)[: N // 10]
    isl[moved] = rng.integers(0, K, len(moved))
    theta = centres[isl] + (LN2 / np.sqrt(D)) * rng.standard_normal((N, D))
    return theta.reshape(N, H, da).astype(np.float32)


def case_sigma_p(case):
    """1.3 ln 2; d_a = 2: 1.3 and 0.8 times it (two prior scales per column parity)"""
    base = 1.3 * LN2
    return np.array([1.3 * base, 0.8 * base], np.float32) if case["da"] == 2 else np.array([base], np.float32)


def _input_key(case):
    return (case["model"], case["N"], case["D"], case["family"], case["weights"], case["seed"])


def case_inputs(case):
    """dict(theta [N, H, da] fp32, mix [N] fp32 normalised, sigma_p [da] fp32) - read-only arrays, one set per input key"""
    return _inputs(_input_key(case))


@functools.lru_cache(maxsize=None)
def _inputs(key):
    case = next(c for c in ALL_CASES if _input_key(c) == key)
    N, H, da, D = case["N"], case["H"], case["da"], case["D"]
    rng = np.random.default_rng(case["seed"])
    sp = case_sigma_p(case)
    if case["family"] == "islands":
        theta = islands(rng, N, H, da, sp)
    else:
        theta = cloud(rng, N, H, da, 1.0, rng.standard_normal(D).astype(np.float32))
        if case["family"] == "clusters":  # the second half 150 scaled units (squared) away: every block between the halves is far
            theta[N // 2:] += (np.sqrt(150.0 / D) * np.tile(np.broadcast_to(sp, (da,)), H)).reshape(1, H, da).astype(np.float32)
    u = rng.random(N)
    if case["weights"] == "steep":
        mix = np.exp(-6.0 * u).astype(np.float32)
    else:
        mix = (u + 0.05).astype(np.float32)
        if case["weights"] == "zeros":
            mix[:64] = 0.0
            mix[rng.permutation(N)[: N // 10]] = 0.0
    mix = (mix / mix.sum(dtype=np.float64)).astype(np.float32)
    for a in (theta, mix, sp):
        a.setflags(write=False)
    return dict(theta=theta, mix=mix, sigma_p=sp)


# ---- the case table ("log p on large aliased sets at every compiled width")
def dpb_for(D):
    return max(16, 16 * ((D + 15) // 16))


def _case(model, N, D, weights, family="islands", imq=False, seed=None):
    da = 1 if model == "pendulum" else 2
    assert D % da == 0
    cid = "%s-N%d-D%d-%s-%s" % (model[:4], N, D, family, weights)
    return dict(id=cid, model=model, N=N, H=D // da, da=da, D=D, dpb=dpb_for(D), family=family, weights=weights, imq=imq,
                seed=(9000 + 131 * N + D) if seed is None else seed)


# N <= 2304 (under DUST_PAIR_BIG=1): the dense matrix-core pass with and without the pre-pass, and the exact-difference pass.  2048: whole
# 256-query tiles; 2049: a tile and a key chunk of one row; 2111 = 32 * 64 + 63: a last 64-query group of 63; every width at a ragged N
# and at 2048; odd D Pendulum, even D Particle (two prior scales), Pendulum at D = 16 and 48 as well.
SMALL_CASES = [
    _case("particle", 2048, 16, "flat", seed=280304), _case("pendulum", 2111, 16, "steep"),
    _case("pendulum", 2049, 17, "zeros"), _case("particle", 2048, 32, "steep"),
    _case("pendulum", 2111, 33, "steep"), _case("pendulum", 2048, 48, "flat", seed=282336), _case("particle", 2304, 48, "flat"),
    _case("pendulum", 2049, 49, "flat"), _case("particle", 2048, 64, "zeros"), _case("particle", 2111, 64, "steep"),
    _case("pendulum", 2111, 65, "flat"), _case("particle", 2048, 80, "steep"),
    _case("particle", 2304, 48, "flat", family="dense"), _case("pendulum", 2049, 33, "flat", family="clusters"),
]
# 8192 <= N <= 16384: the run-list pass (tile order, index order, behind an IMQ pass 1) and the matrix-core pass without the pre-pass.
# 8193: a last group of one query and a last chunk of one key; every width at 8192 or 8193 / 8255; eight cases, one at 16384.
LARGE_CASES = [
    _case("particle", 8192, 48, "flat", imq=True), _case("pendulum", 8193, 17, "steep", imq=True),
    _case("particle", 8255, 64, "steep", imq=True, seed=1091469), _case("particle", 8192, 80, "zeros", imq=True),
    _case("particle", 8193, 16, "flat", family="dense", imq=True), _case("pendulum", 8255, 65, "flat", family="clusters"),
    _case("pendulum", 12305, 33, "zeros"), _case("particle", 16384, 32, "flat"),
]
ALL_CASES = SMALL_CASES + LARGE_CASES
assert len({c["id"] for c in ALL_CASES}) == len(ALL_CASES)
assert sum(c["N"] >= 8192 for c in ALL_CASES) <= 8 and sum(c["N"] == 16384 for c in ALL_CASES) <= 1
DECIDE_CASE_ID = "part-N2304-D48-dense-flat"  # the pre-pass decision test: a dense cloud with far share 0

# variants that cannot show at a case, with the reason (the CPU module asserts that each listed one is indeed under the 10-tolerance line)
_DENSE_LAST = ("the last key carries ~1 / (N E k) of a dense row's sum (E k ~ 0.4: every key is a neighbour of every query): "
               "measured 2 ... 8 tolerances")
NOT_APPLICABLE = {
    "part-N2304-D48-dense-flat": {"drop_last": _DENSE_LAST},
    "part-N8193-D16-dense-flat": {"drop_last": _DENSE_LAST},
    "pend-N8255-D65-clusters-flat": {"drop_last": _DENSE_LAST},  # (a dense half of 4127)
}


def logp_variants(case):
    """The variants that can show in log p at a case.  swap_sigma needs two scales.  drop_last moves the last row's value (and its
    island's) by the last key's share of those sums: with an exact-zero weight - clamped to 2^-23 by log_mix - the share is ~1e-7 of a
    neighbour's and the variant cannot show."""
    out = [v for v in LOGP_VARIANTS if v != "swap_sigma" or case["da"] == 2]
    if case["weights"] == "zeros" and case_inputs(case)["mix"][-1] == 0.0:
        out.remove("drop_last")
    return tuple(v for v in out if v not in NOT_APPLICABLE.get(case["id"], {}))


def case_by_id(cid):
    for c in ALL_CASES:
        if c["id"] == cid:
            return c
    raise KeyError(cid)


def measure(cid):
    """dict(ref [N] float64 log p WITHOUT its constant, log_norm, live [groups, chunks], far_share, absmax (of log p with its constant),
    d_moved, d_prod, tol, power {variant: |variant - ref|max over ALL of LOGP_VARIANTS the shape admits}; N <= 2304 also d32, tol_exact)
    of a case, from the restatements alone: d_moved = |logp_ref(theta moved one fp32 ulp per entry) - ref|max,
    d_prod = |logp_ref(dtype = float32) - ref|max, tol = max(2e-6 (1 + |log p|max), 2 d_moved, 2 d_prod) for the product-form passes;
    tol_exact = max(2e-6 (1 + |log p|max), 2 d_moved, 2 d32) with d32 from prior_ref(dtype = float32) for the exact-difference pass.
    Never computed from device output; one measurement per input set."""
    return _measure(_input_key(case_by_id(cid)))


@functools.lru_cache(maxsize=None)
def _measure(key):
    case = next(c for c in ALL_CASES if _input_key(c) == key)
    inp = case_inputs(case)
    th, mix, sp = inp["theta"], inp["mix"], inp["sigma_p"]
    shape_variants = tuple(v for v in LOGP_VARIANTS if v != "swap_sigma" or case["da"] == 2)
    res, live = logp_all(th, mix, sp, variants=shape_variants, live_nats=FAR_NATS)
    ref = res[None]
    ln = log_norm(case["H"], case["da"], sigma_p=sp)
    absmax = float(np.abs(ref + ln).max())
    d_moved = float(np.abs(logp_ref(ulp_moved(th, case["seed"] + 1), mix, sp) - ref).max())
    d_prod = float(np.abs(logp_ref(th, mix, sp, dtype=np.float32).astype(np.float64) - ref).max())
    floor = 2e-6 * (1.0 + absmax)
    out = dict(ref=ref, log_norm=ln, live=live, far_share=float((~live).mean()), absmax=absmax, d_moved=d_moved, d_prod=d_prod,
               tol=max(floor, 2.0 * d_moved, 2.0 * d_prod), power={v: float(np.abs(res[v] - ref).max()) for v in shape_variants})
    if case["N"] <= SMALL_N:
        d32 = float(np.abs(prior_ref(th, th, mix, sigma_p=sp, dtype=np.float32)[1].astype(np.float64) - ref).max())
        out.update(d32=d32, tol_exact=max(floor, 2.0 * d_moved, 2.0 * d32))
    ref.setflags(write=False)
    live.setflags(write=False)
    return out


def reference(case, mix):
    """log p [N] float64 WITH its constant at the mixture weights the context holds: the shared measurement's when they are the case's own"""
    m = measure(case["id"])
    inp = case_inputs(case)
    if np.array_equal(np.asarray(mix), inp["mix"]):
        return m["ref"] + m["log_norm"]
    return logp_ref(inp["theta"], mix, inp["sigma_p"]) + m["log_norm"]
