"""The K1 / IMQ Stein pass and the Gaussian-mixture prior pass beyond the fixtures (TEST INFRASTRUCTURE): float64 numpy restatements with
EXACT differences, seeded inputs whose Gram matrix is DENSE by construction, and the case table shared by tests/test_pairwise_cases_cpu.py
(which pins the restatements and measures every tolerance from them alone) and tests/test_gpu_pairwise_sizes.py (which holds the kernels of
stein.hpp, pairwise_big.hpp, pairwise_fused.hpp + pairwise_packed.hpp, tick2.hpp, fused.hpp and svmpc_batch.hpp to them).  Numpy only:
nothing here imports the reference, the oracle or the library.  The sibling of tests/k2_cases.py.

Why the inputs matter: K1's lengthscale is ln 2.  A cloud `mu + 2 N(0, 1)` in 30 dimensions has pair distances of ~ 15 lengthscales, every
off-diagonal Gram value underflows and phi_i = score_i / N whatever a kernel does with the other keys.  Here theta = centre + c ln2 / sqrt(D)
N(0, 1): the expected squared pair distance is 2 c^2 ln^2 2 - one to two lengthscales - in every dimension count.

A case is a dict: id, row (the implementation's row of the table in DESIGN.md section 2), dev (the kernel that serves it), model, kind
("K1" / "IMQ"), N, H, da, family ("c1", "c15": c = 1 / 1.5; "zeros": mixture weights of keys 0 ... 63 and of a scattered tenth exactly 0;
"offset": a centre of 50 per coordinate; "clusters": two dense clusters 40 lengthscales apart), cov ("diag" / "full"), ell (IMQ), seed.
"""
import functools

import numpy as np

from helpers import elemerr

LN2 = float(np.log(2.0))
IMQ_ELL = 0.9
STEIN_VARIANTS = ("drop_last", "drop_chunk", "stale_score", "rep_over_n", "half_ell")
PRIOR_VARIANTS = ("drop_last", "drop_chunk", "swap_sigma", "uniform_mix")
TOL_FLOOR, TOL_CAP = 1e-5, 5e-5
P_COV = np.array([[1.1, 0.45], [0.45, 0.6]], np.float32)  # the full 2 x 2 prior covariance of the "full" cases, in units of (1.3 c ln 2)^2
F32_EPS = float(np.finfo(np.float32).eps)


def _block(N, D):
    """query rows per block: ~2 MB of float64 differences, which stay in cache"""
    return max(1, (1 << 18) // max(1, N * D))


def _wsum(w, df):
    """sum_j w_ij df_ijd -> [b, D] (a batched matrix product)"""
    return np.matmul(w[:, None, :], df)[:, 0, :]


def _keys(N, variant):
    if variant == "drop_last":
        return np.arange(N - 1)
    if variant == "drop_chunk":
        return np.concatenate([np.arange(min(64, N)), np.arange(128, N)])
    return np.arange(N)


def _gone(N, variant):
    return np.setdiff1d(np.arange(N), _keys(N, variant))


# ---- the Stein pass
def stein_all(theta, score, kind, ell=None, dtype=np.float64, variants=()):
    """{None: phi, variant: phi ...}, each [N, H, da] in `dtype`, in ONE pass over the exact differences df = x_i - x_j:
    K1 (svmpc.py:76-83, gpytorch RBF with lengthscale ln 2): k = exp(-|df|^2 / (2 ln^2 2)), phi_i = sum_j -k df / ln^2 2 + (sum_j k s_j) / N;
    IMQ: k = (1 + |df|^2 / ell^2)^-1/2, dk = -k^3 / ell^2, phi_i = sum_j dk df + (sum_j k s_j) / N.  The repulsion is NOT divided by N.
    Power variants: "drop_last" the last key left out, "drop_chunk" keys 64 ... 127 left out, "stale_score" the score rows rotated by
    one, "rep_over_n" the repulsion divided by N, "half_ell" half the lengthscale."""
    theta = np.asarray(theta)
    shape = theta.shape
    N = shape[0]
    x = theta.reshape(N, -1).astype(dtype)
    s = np.asarray(score).reshape(N, -1).astype(dtype)
    D = x.shape[1]
    l0 = dtype(LN2 if kind == "K1" else ell)
    n = dtype(N)
    want = (None,) + tuple(variants)
    out = {v: np.zeros((N, D), dtype) for v in want}
    s_rot = np.roll(s, 1, axis=0)
    B = _block(N, D)

    def weights(d2, l):
        if kind == "K1":
            k = np.exp(-d2 / (dtype(2.0) * l * l))
            return k, -k / (l * l)
        k = dtype(1.0) / np.sqrt(dtype(1.0) + d2 / (l * l))
        return k, -(k * k * k) / (l * l)

    buf = np.empty((B, N, D), dtype)
    gone = {v: _gone(N, v) for v in variants if v in ("drop_last", "drop_chunk")}
    for i0 in range(0, N, B):
        sl = slice(i0, min(i0 + B, N))
        df = buf[: sl.stop - i0]
        np.subtract(x[sl, None, :], x[None, :, :], out=df)  # [b, N, D], exact
        d2 = np.einsum("ijd,ijd->ij", df, df)
        k, w = weights(d2, l0)
        rep, att = _wsum(w, df), k @ s
        out[None][sl] = rep + att / n
        for v in variants:
            if v in gone:
                g = gone[v]
                out[v][sl] = (rep - _wsum(w[:, g], df[:, g, :])) + (att - k[:, g] @ s[g]) / n
            elif v == "stale_score":
                out[v][sl] = rep + (k @ s_rot) / n
            elif v == "rep_over_n":
                out[v][sl] = rep / n + att / n
            elif v == "half_ell":
                k2, w2 = weights(d2, l0 / dtype(2.0))
                out[v][sl] = _wsum(w2, df) + (k2 @ s) / n
            else:
                raise KeyError(v)
    return {v: a.reshape(shape) for v, a in out.items()}


def stein_ref(theta, score, kind, ell=None, dtype=np.float64, variant=None):
    return stein_all(theta, score, kind, ell, dtype, () if variant is None else (variant,))[variant]


def row_mass(theta, kind="K1", ell=None):
    """off-diagonal Gram row sums [N] (float64, exact differences): the density of a cloud as the Stein pass sees it"""
    theta = np.asarray(theta)
    N = theta.shape[0]
    x = theta.reshape(N, -1).astype(np.float64)
    out = np.empty(N)
    B = _block(N, x.shape[1])
    buf = np.empty((B, N, x.shape[1]))
    for i0 in range(0, N, B):
        df = buf[: min(B, N - i0)]
        np.subtract(x[i0:i0 + B, None, :], x[None, :, :], out=df)
        d2 = np.einsum("ijd,ijd->ij", df, df)
        k = np.exp(-d2 / (2.0 * LN2 * LN2)) if kind == "K1" else 1.0 / np.sqrt(1.0 + d2 / (ell * ell))
        out[i0:i0 + B] = k.sum(1) - 1.0
    return out


def median_mass(theta):
    """median K1 row mass of a cloud, the diagonal's 1 included"""
    return 1.0 + (float(np.median(row_mass(theta))) if np.asarray(theta).shape[0] > 1 else 0.0)


def dense_enough(theta):
    """the condition every whole-iteration test asserts on the particles it feeds the reference: median K1 row mass >= min(N, 8) / 2"""
    return median_mass(theta) >= min(np.asarray(theta).shape[0], 8) / 2.0


# ---- the prior pass
def log_mix(mix, dtype=np.float64, clamp=True):
    """log mixture weights [N].  clamp=True: torch's Categorical(probs=) as the reference builds it (probs normalised, clamped to
    [eps, 1 - eps], logged, log-softmaxed): an exact zero weight enters as log(2^-23).  clamp=False: plain log(pi / sum pi), -inf at 0."""
    w = np.asarray(mix).astype(dtype)
    p = w / w.sum()
    if clamp:
        p = np.clip(p, dtype(F32_EPS), dtype(1.0 - F32_EPS))
    with np.errstate(divide="ignore"):
        lg = np.log(p)
    m = lg.max()
    return lg - (m + np.log(np.exp(lg - m).sum()))


def _whiten(x, da, sigma_p, chol_p, dtype):
    """rows [n, D] -> whitened rows: per time step z = L^-1 x by forward substitution (diagonal: x / sigma_{d % da})"""
    n, D = x.shape
    if chol_p is None:
        sg = np.broadcast_to(np.asarray(sigma_p, np.float32).reshape(-1), (da,)).astype(dtype)
        return x / np.tile(sg, D // da)[None, :]
    l00, l10, l11 = (dtype(v) for v in np.asarray(chol_p, np.float32).reshape(-1))
    z = np.empty_like(x)
    z[:, 0::2] = x[:, 0::2] / l00
    z[:, 1::2] = (x[:, 1::2] - l10 * z[:, 0::2]) / l11
    return z


def _unwhiten(g, da, sigma_p, chol_p, dtype):
    """whitened gradient rows -> L^-T g (diagonal: g / sigma)"""
    n, D = g.shape
    if chol_p is None:
        sg = np.broadcast_to(np.asarray(sigma_p, np.float32).reshape(-1), (da,)).astype(dtype)
        return g / np.tile(sg, D // da)[None, :]
    l00, l10, l11 = (dtype(v) for v in np.asarray(chol_p, np.float32).reshape(-1))
    w = np.empty_like(g)
    w[:, 1::2] = g[:, 1::2] / l11
    w[:, 0::2] = (g[:, 0::2] - l10 * w[:, 1::2]) / l00
    return w


def prior_all(theta, mu, mix, sigma_p=None, chol_p=None, dtype=np.float64, variants=(), clamp=True):
    """{None: (grad_pri [N, H, da], log_p_unnormalised [N]), variant: ...} of the mixture sum_k pi_k N(x; mu_k, Sigma_p) (svmpc.py:38-45,
    svgd.py:84-89): logits_ik = log pi_k - 1/2 sum_d ((x_i - mu_k)_d / sigma_{d % da})^2, responsibilities by max-shifted softmax,
    grad_pri_i = sum_k r_ik (mu_k - x_i) / sigma^2, log p = logsumexp_k logits (WITHOUT -H log det - D/2 log 2 pi: `log_norm`).  chol_p
    (l00, l10, l11): a full 2 x 2 covariance per time step - differences whitened by forward substitution, the gradient unwhitened by
    back substitution.  The differences are formed BEFORE the scaling (exact in fp32 for nearby values).  Zero weights with clamp=False
    give -inf logits and no NaN.  Power variants: "drop_last" / "drop_chunk" components left out (last; 64 ... 127), "swap_sigma" the two
    scales exchanged, "uniform_mix" the weights ignored."""
    theta = np.asarray(theta)
    shape = theta.shape
    N, da = shape[0], shape[-1]
    x = theta.reshape(N, -1).astype(dtype)
    y = np.asarray(mu).reshape(N, -1).astype(dtype)
    D = x.shape[1]
    lm = log_mix(mix, dtype, clamp)
    want = (None,) + tuple(variants)
    out = {v: (np.zeros((N, D), dtype), np.zeros(N, dtype)) for v in want}
    B = _block(N, D)
    buf = np.empty((B, N, D), dtype)
    gone = {v: _gone(N, v) for v in variants if v in ("drop_last", "drop_chunk")}

    def softmax_sum(lg, dz):
        """logits [b, K], whitened differences mu_k - x_i [b, K, D] -> (e = exp(lg - max), sum_k e, sum_k e dz [b, D], max)"""
        m = lg.max(1, keepdims=True)
        m = np.where(np.isfinite(m), m, dtype(0.0))  # (a row of -inf logits: no NaN from inf - inf)
        e = np.exp(lg - m)
        return e, e.sum(1, keepdims=True), _wsum(e, dz), m

    def result(z, num, m, sp):
        with np.errstate(divide="ignore", invalid="ignore"):
            return _unwhiten(num / z, da, sp, chol_p, dtype), (m + np.log(z))[:, 0]

    def whitened(sl, sp):
        dz = buf[: sl.stop - sl.start]
        np.subtract(y[None, :, :], x[sl, None, :], out=dz)  # mu_k - x_i, exact
        b = dz.shape[0]
        dz[...] = _whiten(dz.reshape(b * N, D), da, sp, chol_p, dtype).reshape(b, N, D)
        return dz, np.einsum("ikd,ikd->ik", dz, dz)

    for i0 in range(0, N, B):
        sl = slice(i0, min(i0 + B, N))
        dz, q = whitened(sl, sigma_p)
        lg = lm[None] - dtype(0.5) * q
        e, z, num, m = softmax_sum(lg, dz)
        out[None][0][sl], out[None][1][sl] = result(z, num, m, sigma_p)
        for v in variants:
            if v in gone:  # the same sums without the dropped components
                g = gone[v]
                r = result(z - e[:, g].sum(1, keepdims=True), num - _wsum(e[:, g], dz[:, g, :]), m, sigma_p)
            elif v == "uniform_mix":
                e2, z2, num2, m2 = softmax_sum(-np.log(dtype(N)) - dtype(0.5) * q, dz)
                r = result(z2, num2, m2, sigma_p)
            elif v == "swap_sigma":
                continue
            else:
                raise KeyError(v)
            out[v][0][sl], out[v][1][sl] = r
        if "swap_sigma" in variants:
            sp = np.asarray(sigma_p, np.float32).reshape(-1)[::-1]
            dz, q = whitened(sl, sp)
            e, z, num, m = softmax_sum(lm[None] - dtype(0.5) * q, dz)
            out["swap_sigma"][0][sl], out["swap_sigma"][1][sl] = result(z, num, m, sp)
    return {v: (g.reshape(shape), lp) for v, (g, lp) in out.items()}


def prior_ref(theta, mu, mix, sigma_p=None, chol_p=None, dtype=np.float64, variant=None, clamp=True):
    return prior_all(theta, mu, mix, sigma_p, chol_p, dtype, () if variant is None else (variant,), clamp)[variant]


def log_norm(H, da, sigma_p=None, chol_p=None):
    """the constant of the mixture's log-density: -H log det L_p - D / 2 log 2 pi (float64, from the fp32 scales)"""
    if chol_p is not None:
        c = np.asarray(chol_p, np.float32).astype(np.float64).reshape(-1)
        ld = np.log(c[0]) + np.log(c[2])
    else:
        ld = float(np.log(np.broadcast_to(np.asarray(sigma_p, np.float32).reshape(-1), (da,)).astype(np.float64)).sum())
    return float(-H * ld - 0.5 * H * da * np.log(2.0 * np.pi))


def lik_ref(theta, costs, actions, alpha, sigma_a, dtype=np.float64):
    """grad_lik [N, H, da] (svmpc.py:47-54): sum_s softmax_s(-alpha costs[s, i]) (a_si - x_i) / sigma_a^2"""
    theta = np.asarray(theta)
    N, da = theta.shape[0], theta.shape[-1]
    x = theta.reshape(N, -1).astype(dtype)
    a = np.asarray(actions).reshape(actions.shape[0], N, -1).astype(dtype)
    lg = -dtype(np.float32(alpha)) * np.asarray(costs).astype(dtype)  # [S, N]
    e = np.exp(lg - lg.max(0, keepdims=True))
    w = e / e.sum(0, keepdims=True)
    sa = np.broadcast_to(np.asarray(sigma_a, np.float32).reshape(-1), (da,)).astype(dtype)
    s2 = np.tile(sa * sa, x.shape[1] // da)
    return (np.einsum("si,sid->id", w, a - x[None]) / s2[None]).reshape(theta.shape)


def chol2(p_cov):
    """(l00, l10, l11) of a 2 x 2 covariance, rounded to fp32 as the library holds them"""
    L = np.linalg.cholesky(np.asarray(p_cov, np.float32).astype(np.float64))
    return np.array([L[0, 0], L[1, 0], L[1, 1]], np.float32)


def ulp_moved(a, seed):
    """an fp32 array with every entry moved one ulp in a seeded random direction"""
    a = np.asarray(a, np.float32)
    up = np.random.default_rng(seed).integers(0, 2, a.shape).astype(bool)
    return np.where(up, np.nextafter(a, np.float32(np.inf)), np.nextafter(a, np.float32(-np.inf))).astype(np.float32)


# ---- seeded inputs
def cloud(rng, N, H, da, c, centre):
    D = H * da
    return (centre.reshape(1, H, da) + np.float32(c * LN2 / np.sqrt(D)) * rng.standard_normal((N, H, da)).astype(np.float32)).astype(np.float32)


def case_c(case):
    """The width factor c of a case's cloud: 1 (c15: 1.5).  N <= 8: 0.7 of it - the density condition min(N, 8) / 2 asks a row of eight for
    a mean off-diagonal Gram value of 3 / 7 = 0.43, and E k = (1 + 2 c^2 / D)^(-D / 2) -> e^(-c^2) is 0.37 at c = 1, 0.61 at c = 0.7."""
    return (1.5 if case["family"] == "c15" else 1.0) * (0.7 if case["N"] <= 8 else 1.0)


def case_sigma_p(case):
    """the prior scale(s) as the context takes them: 1.3 c ln 2; d_a = 2 and an anisotropic case: 1.3 and 0.8 times it"""
    base = 1.3 * case_c(case) * LN2
    if case["da"] == 2 and case["aniso"]:
        return np.array([1.3 * base, 0.8 * base], np.float32)
    return np.full(case["da"], base, np.float32)


def case_p_cov(case):
    if case["cov"] != "full":
        return None
    return (P_COV * np.float32((1.3 * case_c(case) * LN2) ** 2)).astype(np.float32)


def case_inputs(case):
    """dict(theta, mu, score [N, H, da] fp32, mix [N] fp32, sigma_p [da] fp32, chol_p (3,) fp32 or None).  theta and mu scatter round ONE
    centre ~ N(0, 1)^D with c ln2 / sqrt(D) per coordinate; score = 2 N(0, 1); mix = rand + 0.05, normalised."""
    N, H, da, fam = case["N"], case["H"], case["da"], case["family"]
    rng = np.random.default_rng(case["seed"])
    D = H * da
    centre = rng.standard_normal(D).astype(np.float32)
    if fam == "offset":
        centre = (centre + np.float32(50.0)).astype(np.float32)
    c = case_c(case)
    theta, mu = cloud(rng, N, H, da, c, centre), cloud(rng, N, H, da, c, centre)
    if fam == "clusters":  # the second half of the particles 40 lengthscales away (along every coordinate equally)
        shift = np.float32(40.0 * LN2 / np.sqrt(D))
        theta[N // 2:] += shift
        mu[N // 2:] += shift
    score = (2.0 * rng.standard_normal((N, H, da))).astype(np.float32)
    mix = (rng.random(N) + 0.05).astype(np.float32)
    if fam == "zeros":
        mix[:64] = 0.0
        mix[rng.permutation(N)[: N // 10]] = 0.0
    mix = (mix / mix.sum(dtype=np.float64)).astype(np.float32)
    pc = case_p_cov(case)
    return dict(theta=theta, mu=mu, score=score, mix=mix, sigma_p=case_sigma_p(case), chol_p=None if pc is None else chol2(pc))


# ---- the case table ("K1 / IMQ and the prior beyond the fixtures")
def cpt_for(D):
    return 4 if D <= 32 else (8 if D <= 64 else (12 if D <= 96 else 16))


def pair_geometry(N, big=False, D=30):
    """(tiles, JS, slice, chunks per slice) of the tiled pairwise launches: a pure-Python copy of the arithmetic of `pair_geometry`
    (dust_amd.hip) for an unsharded context without the fused large-set pass - query tiles of 32 (large-set kernel: 4096 / DPB), 64-key
    chunks, at least ~512 workgroups where the chunks allow."""
    ti = (4096 // (32 if D <= 32 else 64)) if big else 32
    tiles = (N + ti - 1) // ti
    chunks = (N + 63) // 64
    js = max(1, min((512 + tiles - 1) // tiles, chunks))
    cps = (chunks + js - 1) // js
    sl = cps * 64
    return tiles, (N + sl - 1) // sl, sl, cps


def _case(row, dev, model, kind, N, D, family="c1", cov="diag", aniso=None, **extra):
    da = 1 if model == "pendulum" else 2
    assert D % da == 0
    aniso = (da == 2) if aniso is None else aniso
    cid = "%s-%s-%s-N%d-D%d-%s%s" % (row, model[:4], kind, N, D, family, "-full" if cov == "full" else "")
    for k in sorted(extra):
        cid += "-%s%s" % (k, extra[k])
    c = dict(id=cid, row=row, dev=dev, model=model, kind=kind, N=N, H=D // da, da=da, D=D, family=family, cov=cov, aniso=aniso,
             ell=IMQ_ELL if kind == "IMQ" else None, seed=7000 + 131 * N + D + (17 if kind == "IMQ" else 0))
    c.update(extra)
    return c


def _pw(model, kind, N, D, **kw):
    return _case("pairwise", "pairwise_kernel<., %d>" % cpt_for(D), model, kind, N, D, **kw)


PAIR_N = (1, 2, 31, 32, 33, 63, 64, 65, 97, 1000, 1024, 1025, 1056, 2047, 2048)
PAIR_N_REDUCED = (33, 65, 1056)
PAIR_D = (1, 3, 32, 33, 64, 65, 80, 96, 97, 128)

PAIR_CASES = [_pw("pendulum", "K1", n, 30) for n in PAIR_N]
for _d in PAIR_D:
    for _n in PAIR_N_REDUCED:
        PAIR_CASES.append(_pw("pendulum", "K1", _n, _d))
        if _d % 2 == 0:
            PAIR_CASES.append(_pw("particle", "K1", _n, _d))
PAIR_CASES += [_pw("particle", "K1", _n, 2) for _n in PAIR_N_REDUCED]
PAIR_CASES += [_pw("pendulum", "IMQ", _n, 30) for _n in (33, 65, 1056, 2047)]
PAIR_CASES += [_pw("particle", "K1", _n, 30, cov="full") for _n in (33, 97)]
PAIR_CASES += [_pw("pendulum", "K1", _n, 30, family=_f) for _n in (97, 1056) for _f in ("zeros", "offset", "c15")]

BIG_CASES = [_case("big", "pairwise_big_kernel<., %d>" % (32 if _d <= 32 else 64), "pendulum" if _d == 30 else "particle", _k, _n, _d)
             for _n in (2048, 2049, 2200) for _d in (30, 40) for _k in ("K1", "IMQ")]

BIG_CASES.append(_case("big", "pairwise_big_kernel<., 32>", "pendulum", "K1", 2048, 30, family="clusters"))  # (a case that rejects stale_score)

FUSEDBIG_CASES = [_case("fusedbig", "pairwise_packed_kernel", "pendulum" if _d == 30 else "particle", "K1", _n, _d, far=_far)
                  for _n in (2048, 2100) for _d in (30, 80) for _far in ("default", "0")]
FUSEDBIG_CASES.append(_case("fusedbig", "pairwise_packed_kernel + pairwise_far", "pendulum", "K1", 2048, 30, family="clusters", far="default"))

TICK2_N = (4, 8, 36, 60, 64, 68, 100, 1000, 1024)
TICK2_CASES = [_case("tick2", "svmpc_tick2_kernel", "pendulum", "K1", _n, 30) for _n in TICK2_N]
TICK2_CASES += [_case("tick2", "svmpc_tick2_kernel", "pendulum", _k, _n, _d) for _d in (1, 32) for _n in (36, 100) for _k in ("K1", "IMQ")]
TICK2_CASES += [_case("tick2", "svmpc_tick2_kernel", "pendulum", "IMQ", _n, 30) for _n in (68, 1000)]
TICK2_CASES += [_case("tick2", "svmpc_tick2_kernel", "particle", "K1", _n, _d, aniso=False) for _d in (2, 32) for _n in (36, 100)]
TICK2_CASES.append(_case("tick2", "svmpc_tick2_kernel", "pendulum", "K1", 100, 30, weighted=1))

FUSED_CASES = [_case("fused", _dev, "pendulum", "K1", _n, _d, path=_p) for _n in (36, 64, 100, 1000, 1024) for _d in (30, 64)
               for _p, _dev in (("nofuse", "fused_prior_rollout_kernel + stein_update_kernel / svgd_iter_kernel"),
                                ("plain", "pairwise_kernel + update_kernel (the plain chain)"))]

BATCH_CASES = [_case("batch", "svmpc_batch_kernel", "pendulum", _k, _n, _d) for _n in (1, 2, 3, 33, 63, 64) for _d in (1, 30, 33, 128)
               for _k in ("K1", "IMQ") if _k == "K1" or _d in (30, 128)]
BATCH_CASES.append(_case("batch", "svmpc_batch_kernel", "particle", "K1", 33, 30))  # (two prior scales: inv_sp per column)

ALL_CASES = PAIR_CASES + BIG_CASES + FUSEDBIG_CASES + TICK2_CASES + FUSED_CASES + BATCH_CASES
del _d, _n
assert len({c["id"] for c in ALL_CASES}) == len(ALL_CASES)
ALIASED_ROWS = ("fusedbig", "tick2", "fused")  # rows whose prior means ARE the particles


def stein_variants(case):
    """The Stein variants that can show at a case's shape.  One particle has no pair: a dropped key is the only error there is.  The chunk
    of keys 64 ... 127 exists from N = 65 on.  stale_score: the attraction (sum_j k_ij s_j) / N averages the iid scores of the row's
    neighbours, so rotating them moves phi by ~ 2 sqrt(2 sum_j k_ij^2) / N, while the repulsion - which sets phi's RMS - does not shrink
    with N.  Measured from the restatement: 2.3e-4 ... 3e-4 of the RMS at N = 1000 ... 1056 (D >= 3), 8e-5 ... 1e-4 at N = 2047 ... 2200
    (8 to 10 tolerances) and 2.6e-5 in ONE dimension at N = 1056 (680 neighbours per row): there the variant is below the 10-tolerance
    line of the power condition and does not count as applicable - except in the two-cluster family, whose rows average half as many."""
    N = case["N"]
    if N == 1:
        return ("drop_last",)
    out = [v for v in STEIN_VARIANTS if v != "drop_chunk" or N > 64]
    if not ((N <= 1056 and (case["D"] > 1 or N <= 100)) or case["family"] == "clusters"):
        out.remove("stale_score")
    return tuple(out)


def prior_variants(case):
    """one component: nothing to drop or reweigh; swap_sigma needs two different scales (not the full covariance's own metric);
    a weighted case ("weighted") gets its weights from the device - uniform_mix is checked there on those"""
    N = case["N"]
    if N == 1:
        return ()
    out = [v for v in PRIOR_VARIANTS if v != "drop_chunk" or N > 64]
    if not (case["da"] == 2 and case["aniso"] and case["cov"] == "diag"):
        out.remove("swap_sigma")
    return tuple(out)


def case_by_id(cid):
    for c in ALL_CASES:
        if c["id"] == cid:
            return c
    raise KeyError(cid)


def _prior_args(case, inp):
    mu = inp["theta"] if case["row"] in ALIASED_ROWS else inp["mu"]
    if inp["chol_p"] is not None:
        return mu, dict(chol_p=inp["chol_p"])
    return mu, dict(sigma_p=inp["sigma_p"])


def moved(case, theta):
    """theta (float64) with every entry moved one fp32 ulp in a seeded random direction.  The "offset" family: one ulp OF THE DEVIATION
    from the centre of 50 (theta - 50 is exact in fp32).  An ulp at 50 is 3.8e-6, 3e-5 of the cloud's width of ln2 / sqrt(D): a
    perturbation of the INPUT, which the device never sees - it is handed the very fp32 values the reference reads - and which would let
    the family pass at 9e-5.  What the family is there to show is that exact differences do not care about the centre: it is held to what
    the same cloud measures without its offset, the 1e-5 floor."""
    if case["family"] != "offset":
        return ulp_moved(theta, case["seed"] + 1).astype(np.float64)
    dev = (np.asarray(theta, np.float32) - np.float32(50.0)).astype(np.float32)
    assert np.array_equal(dev.astype(np.float64) + 50.0, np.asarray(theta, np.float64))
    return np.asarray(theta, np.float64) + (ulp_moved(dev, case["seed"] + 1).astype(np.float64) - dev.astype(np.float64))


def _input_key(case):
    return (case["row"] in ALIASED_ROWS, case["model"], case["kind"], case["N"], case["D"], case["family"], case["cov"], case["aniso"])


def measure(cid):
    """dict(d_phi, tol_phi, d_pri, tol_pri, d_logp, tol_logp, power_phi, power_pri, power_logp, mass) of a case, from the restatements
    alone (the project's rule): d = max(elemerr(ref(theta moved one fp32 ulp per entry), ref), elemerr(ref(dtype =
    float32), ref)), tol = max(1e-5, 2 d); log p absolutely: max(2e-6 (1 + |log p|max), 2 d_abs) with log p INCLUDING its constant, as
    the device returns it.  Never computed from device output.  The rows whose prior means alias the particles are measured so.  Cases
    with the same inputs (the seed depends on N, D and the kernel only) share one measurement."""
    return _measure(_input_key(case_by_id(cid)))


@functools.lru_cache(maxsize=None)
def _measure(key):
    case = next(c for c in ALL_CASES if _input_key(c) == key)
    inp = case_inputs(case)
    th, sc = inp["theta"], inp["score"]
    kind, ell = case["kind"], case["ell"]
    th_m = moved(case, th)
    st = stein_all(th, sc, kind, ell, variants=stein_variants(case))
    ref = st[None]
    d_phi = max(elemerr(stein_ref(th_m, sc, kind, ell), ref), elemerr(stein_ref(th, sc, kind, ell, dtype=np.float32), ref))
    tol_phi = max(TOL_FLOOR, 2.0 * d_phi)
    mu, kw = _prior_args(case, inp)
    aliased = case["row"] in ALIASED_ROWS
    pr = prior_all(th, mu, inp["mix"], variants=prior_variants(case), **kw)
    g, lp = pr[None]
    gm, lpm = prior_ref(th_m, th_m if aliased else mu, inp["mix"], **kw)
    g32, lp32 = prior_ref(th, mu, inp["mix"], dtype=np.float32, **kw)
    d_pri = max(elemerr(gm, g), elemerr(g32, g))
    if case["N"] == 1 and aliased:  # (one particle that is its own prior mean: grad_pri is exactly 0)
        d_pri = float(max(np.abs(gm).max(), np.abs(g32).max()))
    d_logp = float(max(np.abs(lpm - lp).max(), np.abs(lp32 - lp).max()))
    ln = log_norm(case["H"], case["da"], **kw)
    tol_logp = max(2e-6 * (1.0 + float(np.abs(lp + ln).max())), 2.0 * d_logp)
    return dict(d_phi=d_phi, tol_phi=tol_phi, d_pri=d_pri, tol_pri=max(TOL_FLOOR, 2.0 * d_pri), d_logp=d_logp, tol_logp=tol_logp,
                power_phi={v: elemerr(st[v], ref) for v in stein_variants(case)},
                power_pri={v: elemerr(pr[v][0], g) for v in prior_variants(case)},
                power_logp={v: float(np.abs(pr[v][1] - lp).max()) for v in prior_variants(case)},
                mass=median_mass(th))


def score_tolerance(theta, mu, mix, costs, actions, alpha, sigma_a, seed, lik_only=False, **kw):
    """(d, tol) of score = grad_lik + grad_pri (lik_only: of grad_lik) at GIVEN costs and actions, by measure()'s rule: the float32
    restatement and the restatement at inputs moved by one fp32 ulp - the particles, and the costs too: the device rounds alpha * cost to
    fp32 before its softmax, half an ulp of a logit of |alpha c| (costs of 1e3 at alpha = 1e-2: 5e-7 on every weight, which the signed
    sum over the samples amplifies).  tol = max(1e-5, 2 d), from the restatements alone."""
    def ref(th, cs, dtype):
        g = lik_ref(th, cs, actions, alpha, sigma_a, dtype)
        return g if lik_only else g + prior_ref(th, mu, mix, dtype=dtype, **kw)[0]

    r = ref(theta, costs, np.float64)
    d = max(elemerr(ref(ulp_moved(theta, seed + 1), ulp_moved(costs, seed + 2), np.float64), r), elemerr(ref(theta, costs, np.float32), r))
    return d, max(TOL_FLOOR, 2.0 * d)


def tolerances(case):
    m = measure(case["id"])
    assert m["tol_phi"] <= TOL_CAP and m["tol_pri"] <= TOL_CAP, (case["id"], m["d_phi"], m["d_pri"])
    return m["tol_phi"], m["tol_pri"], m["tol_logp"]
