"""The tick epilogue beyond the 8-particle fixtures (TEST INFRASTRUCTURE): a float64 numpy restatement of SVMPC.get_weights / forward /
roll / update_prior (svmpc.py:128-200, with torch.distributions' Categorical / MixtureSameFamily log-weight construction) and of
MultiDISCO.step (disco.py:393-417), written from the reference's text; the tolerances; an fp32 emulation with switchable wrong variants
(the power check); and the case tables that tests/test_epilogue_cpu.py and tests/test_gpu_epilogue.py iterate.  Numpy only: nothing here
imports the reference, the oracle or the library.

The comparison is STAGE-LOCAL: every stage's float64 value is computed from the fp32 outputs of the stage before it (the device's own
log_l / log_p / p / particles, read back), so the "one ulp of a cost moves a weight by 1e-4" amplification of the whole-tick tests does
not enter and every bound below is a few fp32 roundings.

Tolerances (eps32 = 2^-23, u = eps32 / 2, sp(x) = np.spacing(float32(|x|)); first order in u)
----------------------------------------------------------------------------------------------
Roundings: every single fp32 rounding is entered as ONE full spacing sp(x) - the bound that holds under any rounding mode, and the form
the dominant term is specified in; round-to-nearest uses at most half of it, which is the margin the power check (the fp32 emulation
stays within HALF of every tolerance) relies on.

expf / logf: the ROCm device-library documentation that states their ULP bounds does not ship with the ROCm installation (no document
under the ROCm tree names them; only the bitcode is installed).  ULP_EXP = ULP_LOG = 3 is assumed - the bound the OpenCL C specification sets
for single-precision exp / log, which those device libraries were written to meet - and the CPU power check (numpy's fp32 exp / log
emulation stays within HALF of every tolerance) is what sets the margin.  Both enter only through terms of a few eps32.

sum_term(n) = min(n - 1, 4 sqrt(n)) u: the relative error of a sum of n non-negative fp32 terms in ANY order.  (n - 1) u is the
worst case; 4 sqrt(n) u is the probabilistic bound of Higham & Mary (2019, "A new approach to probabilistic rounding error analysis":
lambda sqrt(n) u with lambda = 4, failing with probability < 1e-3 for independent roundings), which is the smaller one from n = 17 on.

tol_p(lw): RELATIVE bound on p_i = exp(lw_i - lse(lw)) wherever the float64 p_i >= 2^-100 (below that |p_dev - p| <= 2^-100).
  z = sum exp(lw - m): each term carries the rounding of its argument (sp(range), range = min(max lw - min lw, 104): beyond 104
      the term is zero in fp32) and expf's ULP_EXP eps32; an implementation that merges per-wave (max, sum exp) pieces forms each term as
      a product of two such exponentials, so: dz = sum_term(N) + 2 (ULP_EXP eps32 + sp(range)) + eps32
  lz = m + logf(z): dlz = dz + ULP_LOG sp(log N + 1) + sp(lse)              <- the dominant term: log-weights are O(10 .. 1e3)
  p  = expf(lw - lz): tol_p = dlz + sp(max |lw_i - lse| over the compared entries) + ULP_EXP eps32
sum p: |sum_f64(p_dev) - 1| <= tol_p (the float64 sum of the device's entries: every entry is within tol_p relatively).
tol_logmix(mix): ABSOLUTE bound on logmix = log_softmax(log(clamp(mix / sum mix, eps32, 1 - eps32))).
  probs: sum_term(N) + eps32 relative (the sum, the division); logit l = logf(probs): e_l = sum_term(N) + eps32 + ULP_LOG sp(max |l|)
  lzz = lm + logf(sum exp(l - lm)): e_lzz = sum_term(N) + ULP_EXP eps32 + e_l + sp(max l - min l) + ULP_LOG sp(log N + 1) + sp(lzz)
  logmix = l - lzz: tol_logmix = e_l + e_lzz + sp(max |logmix|)
tol_logmix_seen(lp, log_norm): logmix has no getter; it is observed through log p with the prior means >= 40 sigma_p apart and
  theta = mu: every cross term exp(-0.5 * 1600 + 16) underflows to exactly 0, so log_p[i] = fl(logmix[i] + fl(log_norm)): two roundings,
  sp(lp) + sp(log_norm), on top of tol_logmix.
tol_mean(theta): H eps32 max |theta| absolute (a sum of H terms and one division).  Copies (roll under repeat / resample, a_seq,
  disco's next / a_seq / a_mat under argmax and external) are np.array_equal.
tol_average: MultiDISCO.step's average is accumulated in double on the device and by the oracle: one rounding to fp32, sp(|v|),
  plus N 2^-53 sum |a_mat| |a_mix|.

What the power check found (tests/test_epilogue_cpu.py)
-------------------------------------------------------
* "upper clamp missing" is NOT observable in any output: the clamp moves the one logit on it from 0 to log(1 - eps32) = -1.19e-7, the
  log_softmax that follows moves every other entry by that much - at entries of magnitude >= 15.9, whose half ulp is 4.8e-7 - and
  get_prior() reports mixw / sum mixw, which the clamp never touches.  No case table can catch it; the CPU test asserts exactly this
  (the variant's deviation is <= 2 eps32 on every case) instead of pretending to.
* "argmax of lw taken before the softmax": exp is non-decreasing, so in float64 it never differs from the argmax of p; in fp32 it differs
  only where two distinct lw round to one p, i.e. inside tol_p, where the reference's own answer is an accident of rounding.  The CPU
  test asserts that it never differs on the case table; the device is held to the first index on exact ties only.
* "log_softmax after the clamp missing" shows only where the clamp bites on many entries (sum of the clamped probs = 1 + k eps32): the
  peaked cases with N >= 1023 catch it, the small ones cannot.
* Existing tolerances that could not tell a listed variant from the right answer: relerr(probs, tick_prior_probs) < 5e-3 / 2e-3
  (test_forward_vs_reference, test_forward) is a tensor-max form on 8-16 particles without a clamped entry - both clamp variants and
  the missing log_softmax pass it; relerr(theta, tick_theta_rolled) < 1e-6 on da = 1 fixtures cannot see "mean over all of D".
"""
import math

import numpy as np

EPS32 = float(np.finfo(np.float32).eps)
U32 = EPS32 / 2
P_FLOOR = 2.0 ** -100
ULP_EXP = 3.0
ULP_LOG = 3.0
LANES, WAVE = 1024, 64  # finalize_kernel's layout: element i sits in lane i % 1024, register row i // 1024, wave (i % 1024) // 64
STRATEGIES = ("repeat", "mean", "resample")


def sp(x):
    return float(np.spacing(np.float32(abs(float(x)))))


def _lse(x):
    m = x.max()
    return m + np.log(np.exp(x - m).sum())


# ------------------------------------------------------------------------------------------------ the restatement (float64)
def weights(log_l, log_p):
    """svmpc.py:137-140, 192: log_w = log_l + log_p IN THE INPUTS' dtype (the reference adds two fp32 tensors), then in float64
    p = exp(log_w - logsumexp(log_w)).  -> (p, i_star = first index of max p, lse)"""
    lw = (np.asarray(log_l) + np.asarray(log_p)).astype(np.float64)
    lse = _lse(lw)
    p = np.exp(lw - lse)
    return p, int(np.argmax(p)), float(lse)


def mixture(w, weighted_prior, eps=EPS32):
    """update_prior svmpc.py:160-170 -> get_gmm -> Categorical(probs=mix): probs = mix / sum, logits = log(clamp(probs, eps, 1 - eps))
    (probs_to_logits; eps is the dtype's, float32 in the reference), MixtureSameFamily.log_prob's log_softmax(logits).
    -> (probs, logmix)"""
    w = np.asarray(w, np.float64)
    mix = w if weighted_prior else np.ones_like(w)
    probs = mix / mix.sum()
    logits = np.log(np.clip(probs, eps, 1.0 - eps))
    return probs, logits - _lse(logits)


def roll(theta, steps, strategy, last_row=None):
    """svmpc.py:142-158: circular roll along H, then the last row from the ROLLED tensor."""
    th = np.roll(np.asarray(theta, np.float64), steps, axis=-2)
    if strategy == "repeat":
        th[..., -1, :] = th[..., -2, :]  # (H = 1: IndexError, as in the reference)
    elif strategy == "resample":
        th[..., -1, :] = np.asarray(last_row, np.float64)
    elif strategy == "mean":
        th[..., -1, :] = th.mean(axis=-2)
    else:
        raise ValueError("{} is an invalid roll strategy.".format(strategy))
    return th


def prior_log_prob(theta, mu, logmix, sigma_p, block=256):
    """MixtureSameFamily(Categorical, Independent(MVN(mu_k, diag sigma_p^2))).log_prob(theta) -> [N]"""
    th = np.asarray(theta, np.float64)
    N, H, da = th.shape
    x, y = th.reshape(N, -1), np.asarray(mu, np.float64).reshape(len(mu), -1)
    s = np.tile(np.broadcast_to(np.asarray(sigma_p, np.float64), (da,)), H)
    norm = -np.log(s).sum() - 0.5 * H * da * math.log(2.0 * math.pi)
    out = np.empty(N)
    lm = np.asarray(logmix, np.float64)
    for i0 in range(0, N, block):
        z = (x[i0:i0 + block, None, :] - y[None]) / s
        lg = lm[None] - 0.5 * (z * z).sum(-1)
        m = lg.max(1, keepdims=True)
        out[i0:i0 + block] = (m + np.log(np.exp(lg - m).sum(1, keepdims=True)))[:, 0] + norm
    return out


def log_norm(H, da, sigma_p):
    s = np.broadcast_to(np.asarray(sigma_p, np.float64), (da,))
    return float(-H * np.log(s).sum() - 0.5 * H * da * math.log(2.0 * math.pi))


def a_mix(eta):
    eta = np.asarray(eta, np.float64)
    return np.exp(eta - _lse(eta))


def disco_step(a_mat, a_mix_, strategy, steps, lo, hi, ext=None):
    """disco.py:396-417 -> (next [steps, da], a_seq [H, da], a_mat [N, H, da]) after the step.  a_mat[argmax] is a VIEW: the in-place
    clamp reaches a_mat; a_seq and a_mat are shifted by `steps` and zero-filled."""
    am = np.array(a_mat, np.float64)
    N, H, da = am.shape
    w = np.asarray(a_mix_, np.float64)
    if strategy == "argmax":
        seq = am[int(np.argmax(w))]
    elif strategy == "average":
        seq = np.einsum("nhd,n->hd", am, w)
    elif strategy == "external" and ext is not None:
        seq = np.array(ext, np.float64)
    else:
        raise ValueError("Invalid value for strategy.")
    lo, hi = np.broadcast_to(np.asarray(lo, np.float64), (da,)), np.broadcast_to(np.asarray(hi, np.float64), (da,))
    np.clip(seq, lo, hi, out=seq)
    nxt = seq[:steps].copy()
    seq = np.roll(seq, -steps, axis=0)
    seq[H - steps:] = 0.0
    am = np.roll(am, -steps, axis=1)
    am[:, H - steps:] = 0.0
    return nxt, seq, am


# ------------------------------------------------------------------------------------------------ tolerances (module docstring)
def sum_term(n):
    return min(n - 1, 4.0 * math.sqrt(n)) * U32


def tol_p(lw):
    lw = np.asarray(lw, np.float64)
    N = lw.size
    lse = _lse(lw)
    rng = min(float(lw.max() - lw.min()), 104.0)
    dz = sum_term(N) + 2.0 * (ULP_EXP * EPS32 + sp(rng)) + EPS32
    dlz = dz + ULP_LOG * sp(math.log(N) + 1.0) + sp(lse)
    d = np.abs(lw - lse)
    cmp = d[np.exp(lw - lse) >= P_FLOOR]
    return dlz + sp(cmp.max()) + ULP_EXP * EPS32


def p_err(got, p64):
    """the largest deviation of `got` from p64 in the units of tol_p: relative where p64 >= 2^-100; below it an absolute deviation of
    2^-100 counts as 1 (so `p_err <= tol` reads "relative within tol, or absolute within 2^-100")"""
    got, p64 = np.asarray(got, np.float64), np.asarray(p64, np.float64)
    big = p64 >= P_FLOOR
    e = 0.0
    if big.any():
        e = float((np.abs(got[big] - p64[big]) / p64[big]).max())
    return e, (float(np.abs(got[~big] - p64[~big]).max()) if (~big).any() else 0.0)


def p_ok(got, p64, tol):
    e, a = p_err(got, p64)
    return e <= tol and a <= P_FLOOR


def tol_logmix(mix, weighted_prior=True):
    probs, lmx = mixture(mix, weighted_prior)
    N = probs.size
    l = np.log(np.clip(probs, EPS32, 1.0 - EPS32))
    e_l = sum_term(N) + EPS32 + ULP_LOG * sp(np.abs(l).max())
    lzz = _lse(l)
    e_lzz = sum_term(N) + ULP_EXP * EPS32 + e_l + sp(l.max() - l.min()) + ULP_LOG * sp(math.log(N) + 1.0) + sp(lzz)
    return e_l + e_lzz + sp(np.abs(lmx).max())


def tol_logmix_seen(lp, lnorm):
    return sp(np.abs(np.asarray(lp, np.float64)).max()) + sp(lnorm)


def tol_mean(theta):
    th = np.asarray(theta, np.float64)
    return th.shape[-2] * EPS32 * float(np.abs(th).max())


def tol_average(a_mat, a_mix_):
    am, w = np.abs(np.asarray(a_mat, np.float64)), np.abs(np.asarray(a_mix_, np.float64))
    v = np.einsum("nhd,n->hd", am, w)
    return np.spacing(np.maximum(v, 1e-30).astype(np.float32)).astype(np.float64) + am.shape[0] * 2.0 ** -53 * v


# ------------------------------------------------------------------------------------------------ fp32 emulation and wrong variants
ORDERS = ("sequential", "pairwise", "per64")
WEIGHT_VARIANTS = ("tie_last", "argmax_lw", "no_lower_clamp", "no_upper_clamp", "no_log_softmax", "mixw_from_lw")
ROLL_VARIANTS = ("repeat_preroll", "mean_all_D", "mean_Hm1", "steps_sign")
DISCO_VARIANTS = ("no_writethrough", "amat_wrap")


def sum32(x, order):
    """fp32 sum of a vector in one of three orders"""
    x = np.asarray(x, np.float32)
    if x.size == 0:
        return np.float32(0)
    if order == "sequential":
        return np.cumsum(x, dtype=np.float32)[-1]  # (numpy's cumsum adds left to right in the accumulator's type)
    if order == "per64":
        n = -(-x.size // 64) * 64
        parts = np.concatenate([x, np.zeros(n - x.size, np.float32)]).reshape(-1, 64)
        return sum32(np.array([sum32(r, "sequential") for r in parts], np.float32), "sequential")
    while x.size > 1:  # pairwise
        if x.size & 1:
            x = np.concatenate([x, np.zeros(1, np.float32)])
        x = (x[0::2] + x[1::2]).astype(np.float32)
    return x[0]


def epilogue32(log_l, log_p, weighted_prior, order="sequential", variant=None):
    """The weights / argmax / mixture part in fp32 numpy arithmetic, as a straightforward implementation computes it.
    -> dict(p, i_star, mixw, probs (as get_prior reports: mixw / sum mixw), logmix)"""
    f = np.float32
    lw = (np.asarray(log_l, f) + np.asarray(log_p, f)).astype(f)
    m = lw.max()
    z = sum32(np.exp((lw - m).astype(f)).astype(f), order)
    lz = f(m + np.log(f(z)))
    p = np.exp((lw - lz).astype(f)).astype(f)
    if variant == "tie_last":
        i_star = int(p.size - 1 - np.argmax(p[::-1]))
    elif variant == "argmax_lw":
        i_star = int(np.argmax(lw))
    else:
        i_star = int(np.argmax(p))
    mixw = (lw if variant == "mixw_from_lw" else p) if weighted_prior else np.ones_like(p)
    s = sum32(mixw, order)
    probs = (mixw / s).astype(f)
    lo = f(0.0) if variant == "no_lower_clamp" else f(EPS32)
    hi = f(1.0) if variant == "no_upper_clamp" else f(1.0) - f(EPS32)
    with np.errstate(divide="ignore", invalid="ignore"):
        l = np.log(np.clip(probs, lo, hi)).astype(f)
        if variant == "no_log_softmax":
            logmix = l
        else:
            lm = l.max()
            zs = sum32(np.exp((l - lm).astype(f)).astype(f), order)
            logmix = (l - f(lm + np.log(f(zs)))).astype(f)
        rep = (mixw.astype(np.float64) / mixw.astype(np.float64).sum()).astype(f)
    return dict(p=p, i_star=i_star, mixw=mixw, probs=rep, logmix=logmix)


def roll32(theta, steps, strategy, last_row=None, order="sequential", variant=None):
    th0 = np.asarray(theta, np.float32)
    H, da = th0.shape[-2:]
    th = np.roll(th0, -steps if variant == "steps_sign" else steps, axis=-2).copy()
    if strategy == "repeat" and H >= 2:
        th[..., -1, :] = th0[..., H - 2, :] if variant == "repeat_preroll" else th[..., -2, :]
    elif strategy == "resample":
        th[..., -1, :] = np.asarray(last_row, np.float32)
    elif strategy == "mean":
        flat = th.reshape(-1, H, da)
        out = np.empty((flat.shape[0], da), np.float32)
        for n in range(flat.shape[0]):
            for c in range(da):
                if variant == "mean_all_D":
                    out[n, c] = sum32(flat[n].reshape(-1), order) / np.float32(H * da)
                else:
                    out[n, c] = sum32(flat[n, :, c], order) / np.float32(H - 1 if variant == "mean_Hm1" else H)
        th[..., -1, :] = out.reshape(th[..., -1, :].shape)
    return th


def disco32(a_mat, a_mix_, strategy, steps, lo, hi, ext=None, variant=None):
    am = np.array(a_mat, np.float32)
    N, H, da = am.shape
    lo, hi = np.broadcast_to(np.asarray(lo, np.float32), (da,)), np.broadcast_to(np.asarray(hi, np.float32), (da,))
    if strategy == "argmax":
        i = int(np.argmax(np.asarray(a_mix_, np.float32)))
        seq = np.clip(am[i], lo, hi)
        if variant != "no_writethrough":
            am[i] = seq
    elif strategy == "average":
        seq = np.clip(np.einsum("nhd,n->hd", am.astype(np.float64), np.asarray(a_mix_, np.float64)).astype(np.float32), lo, hi)
    else:
        seq = np.clip(np.asarray(ext, np.float32), lo, hi)
    nxt = seq[:steps].copy()
    seq = np.roll(seq, -steps, axis=0)
    seq[H - steps:] = 0
    am = np.roll(am, -steps, axis=1)
    if variant != "amat_wrap":
        am[:, H - steps:] = 0
    return nxt, seq, am


# ------------------------------------------------------------------------------------------------ ties
def tie_members(kind, N):
    """Indices (i < j) of an exact tie of the maximum, by finalize_kernel's layout; None where N has no such pair.
    a: two lanes of one wave; b: two waves; c: the same lane in register rows 0 and 1; d: index 0 and index N - 1."""
    if kind == "a":
        base = (N - 1) // 2 // WAVE * WAVE
        return None if N < 4 else ((base + 1, base + 3) if base + 3 < N else (1, 3))
    if kind == "b":
        return (5, 5 + 3 * WAVE) if N > 5 + 3 * WAVE else ((2, WAVE + 2) if N > WAVE + 2 else None)
    if kind == "c":
        return (min(7, N - LANES - 1), LANES + min(7, N - LANES - 1)) if N > LANES else None
    if kind == "d":
        return (0, N - 1) if N >= 2 else None
    raise ValueError(kind)


def place(i):
    """(register row, wave, lane) of element i in finalize_kernel"""
    return i // LANES, (i % LANES) // WAVE, i % WAVE


# ------------------------------------------------------------------------------------------------ the cases
FINALIZE_N = (1, 2, 63, 64, 65, 1023, 1024, 1025, 2049, 4095, 4096, 16383, 16384)  # the launch path, D = 3
TICK2_N = (4, 64, 68, 1020, 1024)
BATCH_N = (1, 2, 63, 64)


def synth_log_weights(N, kind, seed, tie=None):
    """(log_l, log_p) fp32 [N] of a CPU case.  flat: a spread of 8 nats around -310 (every p is compared relatively); peaked: one
    particle 60 nats above a 300-nat spread (one probability on each clamp, underflowing entries); tie: flat, with the members of
    `tie` exactly equal and 2 nats above every other entry."""
    rng = np.random.default_rng(seed)
    f = np.float32
    log_p = (-12.5 + 0.25 * rng.standard_normal(N)).astype(f)
    if kind == "peaked":
        log_l = (-600.0 + 300.0 * rng.random(N)).astype(f)
        log_l[rng.integers(N)] = f(-240.0)
    else:
        log_l = (-300.0 + 8.0 * rng.random(N)).astype(f)
    if tie is not None:
        log_l[list(tie)] = f(-289.5)
        log_p[list(tie)] = f(-12.25)
    return log_l, log_p


def weight_cases():
    """Every (N, kind, tie) of the three implementations' size lists -> list of dicts(id, N, kind, tie, seed)"""
    out = []
    for N in sorted(set(FINALIZE_N + TICK2_N + BATCH_N)):
        for kind in ("flat", "peaked"):
            if kind == "peaked" and N < 2:
                continue
            out.append(dict(id="%s%d" % (kind, N), N=N, kind=kind, tie=None, seed=1000 + N))
        for t in "abcd":
            tm = tie_members(t, N)
            if tm is not None:
                out.append(dict(id="tie_%s%d" % (t, N), N=N, kind="tie_" + t, tie=tm, seed=2000 + N))
    return out


ROLL_SHAPES = [("pendulum", 1, H) for H in (2, 3, 32, 33, 127, 128)] + [("particle", 2, H) for H in (2, 16, 17, 64)] + [("skid_steer", 2, 9)]
ROLL_N = (1, 7, 130)


def roll_steps(H):
    return (-1, -2, -(H - 1), -H, -(H + 1), 0, 1)


def roll_inputs(N, H, da, seed):
    """theta [N, H, da] with a different scale per control dimension and a trend along H (so a wrong row, a wrong dimension and a
    wrong divisor all move the last row by far more than tol_mean), and a `resample` last row [N, da]"""
    rng = np.random.default_rng(seed)
    th = rng.standard_normal((N, H, da)) + np.linspace(-1.0, 2.0, H)[None, :, None] + 3.0 * np.arange(da)[None, None, :]
    return th.astype(np.float32), (5.0 + rng.standard_normal((N, da))).astype(np.float32)


DISCO_SHAPES = [(N, da) for N in (1, 65, 1025, 4096) for da in (1, 2)]
DISCO_H = 6


def disco_inputs(N, H, da, seed, tie=None):
    """a_mat [N, H, da] (entries beyond the bounds +-1.5), a_mix [N] (a softmax; `tie`: those members exactly equal and the maximum),
    ext [H, da], bounds"""
    rng = np.random.default_rng(seed)
    am = (2.0 * rng.standard_normal((N, H, da))).astype(np.float32)
    eta = rng.standard_normal(N)
    if tie is not None:
        eta[list(tie)] = eta.max() + 1.0
    w = np.exp(eta - eta.max())
    w = (w / w.sum()).astype(np.float32)
    if tie is not None:
        w[list(tie)] = w[tie[0]]
    ext = (2.0 * rng.standard_normal((H, da))).astype(np.float32)
    am[int(np.argmax(w)), 0] = 2.5  # the chosen row has entries beyond either bound
    am[int(np.argmax(w)), H - 1] = -2.75
    return am, w, ext, -1.5, 1.5


# ------------------------------------------------------------------------------------------------ inputs of the device tests
def sigma_for(N):
    """the prior scale of a device case: the lattice below has a pitch of at least 48 sigma_p (and sigma_p <= 2^-9: the constant rows of
    a tie, 0.25 apart per coordinate, are then far apart too)"""
    side = max(2, int(math.ceil(math.sqrt(N))))
    pitch = 3.8 / (side - 1)
    return min(2.0 ** math.floor(math.log2(pitch / 48.0)), 2.0 ** -9), side, pitch


def lattice_theta(N, H, da, seed, n_sat=0):
    """Particles [N, H, da] fp32 whose pairwise distances are >= 48 sigma_for(N) and stay so under two rolls by -1: uniform in [-1.5, 1.5],
    with control dimension 0 of the last two rows on a lattice in [-1.9, 1.9]^2 (the roll keeps those rows for H >= 3).  The LAST n_sat
    rows are instead constant rows 6, 6.25, ..: beyond the pendulum's torque clamp (2) by more than the control noise the tests use, so
    their rollouts and costs are bit-equal while the rows differ - the members of a tie are taken from them."""
    rng = np.random.default_rng(seed)
    _, side, pitch = sigma_for(N)
    th = rng.uniform(-1.5, 1.5, (N, H, da))
    i = np.arange(N)
    if H >= 2:
        th[:, H - 2, 0] = -1.9 + pitch * (i % side)
    th[:, H - 1, 0] = -1.9 + pitch * (i // side)
    for k in range(n_sat):
        th[N - 1 - k] = 6.0 + 0.25 * k
    return th.astype(np.float32)


def min_separation(theta, sigma_p, sample=4096, seed=0):
    """smallest pairwise distance in units of sigma_p (exact for N <= sample, else over a random subset against all)"""
    x = np.asarray(theta, np.float64).reshape(len(theta), -1)
    rows = np.arange(len(x)) if len(x) <= sample else np.random.default_rng(seed).choice(len(x), sample, replace=False)
    best = np.inf
    for i0 in range(0, len(rows), 256):
        r = rows[i0:i0 + 256]
        d2 = ((x[r, None, :] - x[None]) ** 2).sum(-1)
        d2[np.arange(len(r)), r] = np.inf
        best = min(best, float(d2.min()))
    return math.sqrt(best) / float(sigma_p)


def log_l_of(costs, alpha):
    """ExponentiatedUtility.log_prob (likelihoods.py:127-135) in float64: logsumexp_s(-alpha c) - log S"""
    x = -alpha * np.asarray(costs, np.float64)
    m = x.max(0)
    return m + np.log(np.exp(x - m).sum(0)) - math.log(x.shape[0])


def alpha_for(costs, kind, boost=None):
    """The likelihood's alpha that gives probed costs [S, N] the spread a case needs: flat - max - min of log_l is 4 nats; peaked - the
    best particle is 60 nats above the second (+ `boost`: log-weight offsets added per particle)."""
    b = np.zeros(np.asarray(costs).shape[1]) if boost is None else np.asarray(boost, np.float64)

    def measure(a):
        ll = log_l_of(costs, a) + b
        if kind == "flat":
            return float(ll.max() - ll.min()) / 4.0
        s = np.sort(ll)
        return float(s[-1] - s[-2]) / 60.0

    if np.asarray(costs).shape[1] < 2:
        return 1.0
    lo, hi = 1e-12, 1e6
    for _ in range(200):
        mid = math.sqrt(lo * hi)
        if measure(mid) < 1.0:
            lo = mid
        else:
            hi = mid
    return float(np.float32(hi))
