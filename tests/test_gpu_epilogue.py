"""The tick epilogue's three device implementations against the float64 restatement of tests/epilogue_cases.py, stage by stage: the
launch-per-stage kernels of forward.hpp (DUST_NO_TICK2=1), the tail of the one-launch tick (tick2.hpp; `tick_stats()` tells that it
served the call) and the batched tick (svmpc_batch.hpp).  Every stage is fed the device's OWN fp32 outputs of the stage before it, read
back, so the bounds are the few roundings derived in epilogue_cases' docstring.

How the inputs are steered.  lr = 0: an optimiser call leaves the particles where they are and leaves the costs the weights need.  The
particles sit on a lattice whose pitch is >= 48 sigma_p (epilogue_cases.lattice_theta) and the prior means are the particles - or, where
the prior may differ from them (before the first forward: the launch path and the batch), the particles displaced ALONG THE ONE
COORDINATE THE LATTICE DOES NOT USE by sigma_p sqrt(2 g_i): every cross term of the mixture underflows to exactly 0, so
log_p[i] = logmix[i] - g_i + log_norm, the spread of the log-weights is the g_i of the case table (alpha = 1e-4 makes the likelihood a
jitter on top) and - with displacement 0 - log_p shows logmix, which has no getter.  Where the means alias the particles (tick2, the
batch's later ticks) the spread comes from the likelihood: alpha is computed from probed costs (epilogue_cases.alpha_for).  The spread a
case needs is asserted from the device's own log-weights: a case that misses it FAILS.

Ties.  The members must differ as rows (a_seq tells which one won) and have bit-equal log-weights: they are constant rows beyond the
pendulum's torque clamp, with equal noise rows - bit-equal rollouts and costs -, displacement 0 and equal mixture weights.  Every
prior-pass path gives such rows a bit-equal log p (asserted: the device's own log_l + log_p are compared with ==); the launch path runs
the exact-difference prior pass (DUST_LOGP_MFMA=0), on which log p = logmix + log_norm holds to two roundings at every N.

The chosen particle is held to the reference's own rule on the device's own weights - a_seq == theta[first index of max p_dev] - and,
on an exact tie, to the lower member."""
import math

import numpy as np
import pytest

import epilogue_cases as ec

pytestmark = pytest.mark.gpu

STATE = {"pendulum": np.array([0.0, 0.0], np.float32), "particle": np.array([9.0, 9.0, 0.0, 0.0], np.float32)}  # (at rest, upright / on the target: the costs are O(1) and so are their differences - log-weights of modest magnitude)
SIGMA_A = 0.5


def _grid(model):
    if model != "particle":
        return None
    from oracle import grid_4x4_map

    return grid_4x4_map()


def _eps(rng, *shape):
    return np.clip(rng.standard_normal(shape), -3.0, 3.0).astype(np.float32)  # (|sigma_a eps| <= 1.5: a constant row of 6 stays beyond the clamp)


def _with_tie(theta, eps, tie):
    """move the two saturated rows lattice_theta(n_sat=2) left at the end to the tie's indices; equal noise rows (axis -3 of eps is N)"""
    if tie is None:
        return theta, eps
    i, j = tie
    N = len(theta)
    order = list(range(N))
    for dst, src in ((i, N - 2), (j, N - 1)):
        k = order.index(src)
        order[dst], order[k] = order[k], order[dst]
    theta = np.ascontiguousarray(theta[order])
    eps = eps.copy()
    eps[..., j, :, :] = eps[..., i, :, :]
    return theta, eps


def _gaps(N, kind, seed, tie):
    """g_i >= 0: how far below the best log-weight each particle is to sit (the CPU cases' generator)"""
    ll, lp = ec.synth_log_weights(N, "flat" if tie is not None else kind, seed, tie)
    lw = ll.astype(np.float64) + lp
    return lw.max() - lw


def _displaced(theta, g, sigma):
    mu = theta.astype(np.float64)
    mu[:, 0, -1 if theta.shape[2] > 1 else 0] += sigma * np.sqrt(2.0 * g)  # (row 0 holds no lattice coordinate for H >= 3)
    return mu.astype(np.float32)


def _check_weights(ll, lp, pw, a_seq, theta_pre, kind=None, tie=None, note=""):
    lw = ll + lp
    p, i_star, _ = ec.weights(ll, lp)
    tol = ec.tol_p(lw)
    rel, ab = ec.p_err(pw, p)
    print("%s N=%d %s: p rel %.3g abs-below-floor %.3g tol %.3g sum-1 %.3g" % (note, lw.size, kind, rel, ab, tol, float(pw.astype(np.float64).sum()) - 1.0))
    assert rel <= tol and ab <= ec.P_FLOOR, (note, rel, ab, tol)
    assert abs(float(pw.astype(np.float64).sum()) - 1.0) <= tol, note
    first = int(np.argmax(pw))
    if a_seq is not None:
        assert np.array_equal(a_seq, theta_pre[first]), (note, first, i_star)
    s = np.sort(lw.astype(np.float64))
    if lw.size > 1 and s[-1] - s[-2] > 4 * tol:
        assert first == i_star, (note, first, i_star)
    if kind == "flat":
        assert (p >= ec.P_FLOOR).all(), "precondition: a flat case compares every entry relatively"
    if kind == "peaked":
        probs = ec.mixture(pw, True)[0]
        assert probs.max() >= 1.0 - ec.EPS32 and probs.min() <= ec.EPS32, "precondition: a peaked case has a probability on each clamp"
    if tie is not None:
        i, j = tie
        assert lw[i] == lw[j] == lw.max() and int((lw == lw.max()).sum()) == 2, "precondition: an exact tie of the maximum (%r)" % (tie,)
        assert pw[i] == pw[j] == pw.max() and first == i == i_star, (note, first, i, j)
        assert not np.array_equal(theta_pre[i], theta_pre[j])
    return p


def _check_probs(probs, pw, wp, note=""):
    want = ec.mixture(pw, wp)[0]
    # get_prior reports mixw / sum mixw, the sum in double: its rounding to fp32 and one fp32 division (+ the spacing of fp32 subnormals)
    assert (np.abs(probs - want) <= 2 * ec.EPS32 * want + 2.0 ** -149).all(), note


def _check_logmix_seen(lp, lnorm, mix, wp, note=""):
    want = ec.mixture(mix, wp)[1]
    tol = ec.tol_logmix(mix, wp) + ec.tol_logmix_seen(lp, lnorm)
    err = float(np.abs(lp.astype(np.float64) - lnorm - want).max())
    print("%s N=%d: logmix through log_p err %.3g tol %.3g" % (note, lp.size, err, tol))
    assert err <= tol, (note, err, tol)


# ================================================================================================ the launch path
def _launch_env(monkeypatch):
    monkeypatch.setenv("DUST_NO_TICK2", "1")
    monkeypatch.setenv("DUST_LOGP_MFMA", "0")


@pytest.mark.parametrize("N", ec.FINALIZE_N)
def test_finalize_kernel_launch_path(N, monkeypatch):
    """finalize_kernel through svmpc_get_weights (keep_prior) and svmpc_forward, D = 3: p, sum p, the chosen row, the returned prior
    probabilities and the logmix the NEXT get_weights sees, for both values of weighted_prior, a flat and a peaked spread, and the ties
    (a) two lanes of a wave (b) two waves (c) one lane's register rows 0 and 1 (d) index 0 and N - 1: the lower index wins.  The roll
    behind it (`repeat`, steps -1) is a copy.  set_prior's logmix (logmix_kernel) is seen through the first log_p on the way."""
    from dust_amd import Context

    _launch_env(monkeypatch)
    H, da, S = 3, 1, 4
    sigma = ec.sigma_for(N)[0]
    lnorm = ec.log_norm(H, da, sigma)
    runs = [("flat", None, wp) for wp in (False, True)] + ([("peaked", None, wp) for wp in (False, True)] if N >= 2 else [])
    runs += [("tie_" + t, ec.tie_members(t, N), False) for t in "abcd" if ec.tie_members(t, N) is not None]
    for kind, tie, wp in runs:
        note = "launch %s wp=%d" % (kind, wp)
        rng = np.random.default_rng(31 * N + len(kind))
        theta, eps = _with_tie(ec.lattice_theta(N, H, da, N, n_sat=2 if tie else 0), _eps(rng, 1, S, N, H, da), tie)
        assert N == 1 or ec.min_separation(theta, sigma, sample=512) >= 40.0
        g = _gaps(N, kind, 1000 + N, tie)
        mu = _displaced(theta, g, sigma)
        w0 = (rng.random(N) + 0.5).astype(np.float32)
        if tie:
            w0[tie[1]] = w0[tie[0]]
        c = Context(model="pendulum", N=N, S=S, M=1, H=H, kernel="K1", lr=0.0, alpha=1e-4, sigma_a=SIGMA_A, sigma_p=sigma, weighted_prior=wp, seed=3)
        c.set_theta(theta)
        c.set_prior(mu, w0)
        c.set_a_mat(theta)
        c.svmpc_optimize(STATE["pendulum"], 1, eps)
        assert np.array_equal(c.get_theta(), theta)
        pw0 = c.svmpc_get_weights()
        ll, lp = c.get_log_weights()
        # set_prior's logmix, through log_p: log_p + g - log_norm = logmix(w0) (the displacement's square is exact to its own rounding:
        # g enters as |theta - mu|^2 / (2 sigma^2), recomputed here from the fp32 arrays the device was given)
        q = ((theta.astype(np.float64) - mu) ** 2).sum((1, 2)) / (2.0 * sigma * sigma)
        want = ec.mixture(w0, True)[1] - q
        tol = ec.tol_logmix(w0) + ec.tol_logmix_seen(lp, lnorm) + 4 * ec.EPS32 * q.max() + ec.sp(np.abs(want).max())
        assert np.abs(lp.astype(np.float64) - lnorm - want).max() <= tol, note
        _check_weights(ll, lp, pw0, None, theta, kind.split("_")[0] if tie is None else None, tie, note + " get_weights")
        means, probs = c.get_prior()
        assert np.array_equal(means, mu), "get_weights keeps the prior"
        _check_probs(probs, w0, True, note)
        a_seq, pw = c.svmpc_forward()
        ll2, lp2 = c.get_log_weights()
        assert np.array_equal(ll2, ll) and np.array_equal(lp2, lp) and np.array_equal(pw, pw0), note
        _check_weights(ll, lp, pw, a_seq, theta, None, tie, note + " forward")
        rolled = c.get_theta()
        assert np.array_equal(rolled, ec.roll(theta, -1, "repeat")), note
        means, probs = c.get_prior()
        assert np.array_equal(means, rolled)
        _check_probs(probs, pw, wp, note)
        c.set_theta(theta)  # the means alias the particles: they follow, and the next log_p shows the logmix the forward wrote
        c.svmpc_get_weights()
        _, lp3 = c.get_log_weights()
        _check_logmix_seen(lp3, lnorm, pw, wp, note + " next")
        c.close()


@pytest.mark.parametrize("iters", [1, 2])
def test_forward_tail_fused_equals_two_launches(iters, monkeypatch):
    """forward's tail as finalize_roll_kernel (one launch, out of place) and as finalize_kernel + roll_kernel (what profile(True)
    forces): the same inputs after 1 and 2 optimiser iterations - the particles end in either buffer of the ping-pong -, every getter
    bit-identical."""
    from dust_amd import Context

    _launch_env(monkeypatch)
    N, S, H = 130, 8, 5
    rng = np.random.default_rng(iters)
    mu = rng.standard_normal((N, H, 1)).astype(np.float32)
    theta = (mu + rng.standard_normal((N, H, 1))).astype(np.float32)
    eps = _eps(rng, iters, S, N, H, 1)
    got = []
    for prof in (False, True):
        c = Context(model="pendulum", N=N, S=S, M=1, H=H, kernel="K1", lr=0.5, alpha=1.0, sigma_a=SIGMA_A, sigma_p=1.0, weighted_prior=True, seed=3)
        c.set_theta(theta)
        c.set_prior(mu)
        c.set_a_mat(theta)
        c.svmpc_optimize(np.array([3.0, 0.0], np.float32), iters, eps)
        pre = c.get_theta()
        if prof:
            c.profile(True)
        a_seq, pw = c.svmpc_forward()
        if prof:
            names = c.profile_get()
            c.profile(False)
        ll, lp = c.get_log_weights()
        means, probs = c.get_prior()
        got.append((pre, a_seq, pw, ll, lp, c.get_theta(), means, probs))
        c.close()
    for a, b in zip(*got):
        assert np.array_equal(a, b)
    pre, a_seq, pw, ll, lp, post = got[0][:6]
    _check_weights(ll, lp, pw, a_seq, pre, note="fused")
    assert np.array_equal(post, ec.roll(pre, -1, "repeat"))
    assert names, "the profiled run must have timed the forward's kernels"


@pytest.mark.parametrize("model,da,H", ec.ROLL_SHAPES)
def test_roll_kernel(model, da, H, monkeypatch):
    """roll_kernel through svmpc_roll at N in {1, 7, 130}: every steps of the table x the three strategies; `repeat` and `resample` are
    copies, `mean` is within tol_mean and a copy in every other row.  Through svmpc_forward_ex (the strategy is the context's) for the
    rollout families.  Adam's three state slots restart with the roll: the step that follows equals, bit for bit, the step a fresh
    context takes from the rolled particles."""
    from dust_amd import Context

    _launch_env(monkeypatch)
    kw = dict(dt=0.1) if model == "skid_steer" else {}
    for N in ec.ROLL_N:
        theta, last = ec.roll_inputs(N, H, da, 10 * H + da + N)
        c = Context(model=model, N=N, S=1, M=1, H=H, kernel="K1", lr=0.1, sigma_a=SIGMA_A, sigma_p=1.0, grid=_grid(model), **kw)
        for steps in ec.roll_steps(H):
            for strategy in ec.STRATEGIES:
                c.set_theta(theta)
                c.svmpc_roll(steps, strategy, last if strategy == "resample" else None)
                got, want = c.get_theta(), ec.roll(theta, steps, strategy, last)
                if strategy == "mean":
                    assert np.array_equal(got[:, :-1], want[:, :-1]) and np.abs(got - want).max() <= ec.tol_mean(theta), (N, steps)
                else:
                    assert np.array_equal(got, want), (N, steps, strategy)
        c.close()
    if model == "skid_steer":
        return
    N, S = 7, 4
    rng = np.random.default_rng(H)
    theta, last = ec.roll_inputs(N, H, da, 99 + H)
    theta = (0.3 * theta).astype(np.float32)
    eps = _eps(rng, 2, S, N, H, da)
    for strategy in ec.STRATEGIES:
        for steps in (-2, -(H + 1)):
            c = Context(model=model, N=N, S=S, M=1, H=H, kernel="K1", lr=0.0, alpha=1e-4 if da == 2 else 1.0, sigma_a=SIGMA_A, sigma_p=1.0,
                        roll_strategy=strategy, grid=_grid(model))
            c.set_theta(theta)
            c.set_prior(theta)
            c.set_a_mat(theta)
            c.svmpc_optimize(STATE[model], 1, eps[:1])
            a_seq, pw = c.svmpc_forward_ex(steps, last if strategy == "resample" else None)
            assert np.array_equal(a_seq, theta[int(np.argmax(pw))])
            got, want = c.get_theta(), ec.roll(theta, steps, strategy, last)
            assert np.array_equal(got[:, :-1], want[:, :-1]) and np.abs(got - want).max() <= (ec.tol_mean(theta) if strategy == "mean" else 0.0)
            c.close()
    # Adam's state restarts
    kw = dict(model=model, N=N, S=S, M=1, H=H, kernel="K1", optimizer="Adam", lr=0.05, alpha=1e-4 if da == 2 else 1.0, sigma_a=SIGMA_A, sigma_p=1.0,
              grid=_grid(model))
    a = Context(**kw)
    a.set_theta(theta)
    a.set_prior(theta)
    a.set_a_mat(theta)
    a.svmpc_optimize(STATE[model], 1, eps[:1])
    moved = a.get_theta()
    assert not np.array_equal(moved, theta)
    a.svmpc_roll(-1, "repeat")
    rolled = a.get_theta()
    assert np.array_equal(rolled, ec.roll(moved, -1, "repeat"))
    am = a.get_a_mat()
    a.svmpc_optimize(STATE[model], 1, eps[1:])
    b = Context(**kw)
    b.set_theta(rolled)
    b.set_prior(theta)  # (a stand-alone roll leaves the prior where it was: the first prior's means)
    b.set_a_mat(am)
    b.svmpc_optimize(STATE[model], 1, eps[1:])
    assert np.array_equal(a.get_theta(), b.get_theta()), "the step after a roll must be a step from zero optimiser state"
    a.close()
    b.close()


def test_roll_kernel_h1(monkeypatch):
    """H = 1: `mean` is the identity.  For `repeat` the reference raises an IndexError (theta[..., -2, :] of a one-row tensor,
    epilogue_cases.roll raises it too); the device's documented behaviour is pinned instead: the row is kept (forward.hpp: `H >= 2`)."""
    from dust_amd import Context

    _launch_env(monkeypatch)
    for model, da in (("pendulum", 1), ("particle", 2)):
        theta, last = ec.roll_inputs(7, 1, da, 5)
        c = Context(model=model, N=7, S=1, M=1, H=1, sigma_a=SIGMA_A, sigma_p=1.0, grid=_grid(model))
        for strategy in ("mean", "repeat"):
            c.set_theta(theta)
            c.svmpc_roll(-1, strategy)
            assert np.array_equal(c.get_theta(), theta), strategy
        with pytest.raises(IndexError):
            ec.roll(theta, -1, "repeat")
        c.set_theta(theta)
        c.svmpc_roll(-1, "resample", last)
        assert np.array_equal(c.get_theta(), ec.roll(theta, -1, "resample", last))
        c.close()


def _weight_vectors(N, rng):
    out = {}
    if N >= 2:
        w = (rng.random(N) + 0.1).astype(np.float32)
        w[rng.choice(N, max(1, N // 3), replace=False)] = 0.0
        w[0] = 1.0
        out["zeros"] = w
    w = np.zeros(N, np.float32)
    w[N // 2] = 1.0
    out["one_hot"] = w
    out["decades12"] = (10.0 ** rng.uniform(-12.0, 0.0, N)).astype(np.float32)
    out["times1e6"] = (1e6 * (rng.random(N) + 0.1)).astype(np.float32)
    return out


@pytest.mark.parametrize("N", [1, 2, 1025, 16384])
def test_logmix_kernel(N, monkeypatch):
    """logmix_kernel through set_prior(mu, w) and svmpc_update_prior(w): exact zeros (the lower clamp), a one-hot vector (the upper
    clamp), 12 decades, weights unnormalised by 1e6; seen through log_p on separated means.  Negative or NaN weights stay refused and
    leave the getters unchanged."""
    from dust_amd import Context
    from dust_amd._lib import DustError

    _launch_env(monkeypatch)
    H, da, S = 3, 1, 2
    sigma = ec.sigma_for(N)[0]
    lnorm = ec.log_norm(H, da, sigma)
    rng = np.random.default_rng(N)
    theta = ec.lattice_theta(N, H, da, N)
    c = Context(model="pendulum", N=N, S=S, M=1, H=H, kernel="K1", lr=0.0, alpha=1e-4, sigma_a=SIGMA_A, sigma_p=sigma, weighted_prior=True, seed=3)
    c.set_theta(theta)
    c.set_prior(theta)
    c.set_a_mat(theta)
    c.svmpc_optimize(STATE["pendulum"], 1, _eps(rng, 1, S, N, H, da))

    def seen():
        c.svmpc_get_weights()
        return c.get_log_weights()[1]

    for name, w in _weight_vectors(N, rng).items():
        for how in ("set_prior", "update_prior"):
            if how == "set_prior":
                c.set_prior(theta, w)
            else:
                c.set_prior(theta)
                c.svmpc_update_prior(w)
            _check_probs(c.get_prior()[1], w, True, name)
            lp = seen()
            _check_logmix_seen(lp, lnorm, w, True, "%s %s" % (how, name))
            if name in ("zeros", "one_hot") and N >= 2:
                assert ec.mixture(w, True)[1].min() < -15.0, "precondition: an entry on the lower clamp"
    (means0, probs0), lp0 = c.get_prior(), seen()
    for bad in (-1.0, float("nan")):
        w = np.ones(N, np.float32)
        w[N // 2] = bad
        with pytest.raises(DustError):
            c.set_prior(theta + 1.0, w)
        with pytest.raises(DustError):
            c.svmpc_update_prior(w)
    means1, probs1 = c.get_prior()
    assert np.array_equal(means1, means0) and np.array_equal(probs1, probs0) and np.array_equal(seen(), lp0)
    c.close()


@pytest.mark.parametrize("N,da", ec.DISCO_SHAPES)
def test_disco_step_kernels(N, da, monkeypatch):
    """amix_kernel, disco_step_kernel and amat_roll_kernel through disco_forward + disco_step: steps in {1, 2, H}, the three strategies,
    bounds that clamp entries of the chosen row (a_mat shows the write-through), an a_mix tie (across waves where N allows) with the
    lower index winning, `average` against the float64 weighted sum.  dust_disco_step's scratch for `next` holds steps * da floats at
    every shape (at N = 1 the context's scratch of S * N floats is smaller than that: the entry sizes it)."""
    from dust_amd import Context

    _launch_env(monkeypatch)
    model = "pendulum" if da == 1 else "particle"
    H, S = ec.DISCO_H, 4
    tie = ec.tie_members("b", N) or ec.tie_members("d", N)
    am, _, ext, lo, hi = ec.disco_inputs(N, H, da, 3 * N + da)
    am = (0.5 * am).astype(np.float32)
    rng = np.random.default_rng(N + da)
    temp = 1.0
    c = Context(model=model, N=N, S=S, M=1, H=H, temperature=temp, alpha=1.0 / temp, sigma_a=SIGMA_A, min_a=lo, max_a=hi, grid=_grid(model), seed=5)
    actions = (am[None] + SIGMA_A * _eps(rng, S, N, H, da)).astype(np.float32)
    st = STATE[model]
    if tie:  # the best particle's samples copied to the tie's members: equal costs, equal eta, a_mat rows that differ
        c.set_a_mat(am)
        c.disco_forward(st, actions)
        best = int(np.argmax(c.get_a_mix()))
        actions[:, list(tie)] = actions[:, [best]]
    c.set_a_mat(am)
    costs, _, _, _ = c.disco_forward(st, actions)
    mix = c.get_a_mix()
    # a_mix = softmax_n(eta) (disco.py:393), in float64 from the device's costs
    # eta has no getter and is the ROLLOUT kernel's output, not this stage's: it is rebuilt from the device's costs, and the fp32 error of the
    # upstream form eta_n = -cmin_n / temp + logf(sum_s expf(-(c_sn - cmin_n) / temp)) (rollout.hpp; the reference shifts by the global
    # beta = costs.min() instead, disco.py:380-383, which cancels in a_mix) is the uncertainty of this stage's input
    cmin = costs.astype(np.float64).min(0)
    xs = -(costs.astype(np.float64) - cmin) / temp
    eta = -cmin / temp + np.log(np.exp(xs).sum(0))
    d_eta = ec.sp(np.abs(cmin / temp).max()) + ec.sp(np.abs(eta).max()) + 2 * ec.sp(np.abs(xs).max()) + ec.sum_term(S) + ec.ULP_EXP * ec.EPS32 + \
        ec.ULP_LOG * ec.sp(math.log(S) + 1.0)
    tol = ec.tol_p(eta) + 2 * d_eta  # (an error d of the inputs moves a softmax by up to 2 d relatively)
    rel, ab = ec.p_err(mix, ec.a_mix(eta))
    print("disco N=%d da=%d a_mix rel %.3g tol %.3g" % (N, da, rel, tol))
    assert rel <= tol and ab <= ec.P_FLOOR and abs(float(mix.astype(np.float64).sum()) - 1.0) <= tol
    first = int(np.argmax(mix))
    if tie:
        members = sorted(set(tie) | {best})
        assert all(mix[k] == mix.max() for k in members) and first == members[0], (first, members)
    am2 = am.copy()
    am2[first, 0] = 2.5
    am2[first, H - 1] = -2.75
    c.set_a_mat(am2)
    for steps in (1, 2, H):
        for strat in ("argmax", "average", "external"):
            cc = c.clone()
            nxt = cc.disco_step(strat, steps, ext if strat == "external" else None)
            wn, ws, wa = ec.disco_step(am2, mix, strat, steps, lo, hi, ext)
            seq, mat = cc.get_a_seq(), cc.get_a_mat()
            cc.close()
            if strat == "average":
                t = ec.tol_average(am2, mix)
                assert (np.abs(nxt - wn) <= t[:steps]).all() and (np.abs(seq - ws) <= np.roll(t, -steps, axis=0)).all(), (steps, strat)
            else:
                assert np.array_equal(nxt, wn) and np.array_equal(seq, ws), (steps, strat)
            assert np.array_equal(mat, wa), (steps, strat)
            if strat == "argmax" and steps < H:
                assert np.abs(mat[first]).max() <= hi and np.abs(am2[first, steps:]).max() > hi  # the write-through was visible
    c.close()


# ================================================================================================ the one-launch tick
TICK2_RUNS = [(m, N, wp, st, kind, None) for m, st in (("pendulum", "repeat"), ("particle", "mean")) for N in ec.TICK2_N
              for wp, kind in ((False, "flat"), (True, "peaked"))]
TICK2_RUNS += [("pendulum", N, wp, "mean", kind, None) for N, wp, kind in ((64, True, "flat"), (1020, False, "peaked"))]
TICK2_RUNS += [("pendulum", N, True, "repeat", "flat", t) for N in (68, 1024) for t in "abd"]


@pytest.mark.parametrize("model,N,wp,strategy,kind,tie", TICK2_RUNS)
def test_tick2_tail(model, N, wp, strategy, kind, tie):
    """The tail of the one-launch tick on the default path: ticks 2 and 3 of a context (`tick_stats()["tick2"]` counts each of them;
    tick 1 runs plain kernels and only aliases the prior).  lr = 0, so the particles before a tick's roll are the ones read before
    the tick; log_l / log_p are the forward's own.  p, sum p, the chosen row, the roll (`repeat`; `mean` at da = 2 on Particle), the
    returned prior probabilities, and - through the NEXT tick's log_p - the logmix this tick wrote (tick 2 reads tick 1's or
    svmpc_update_prior's, tick 3 reads the one tick 2's kernel wrote).  Ties (a) (b) (d): weighted prior, the members' mixture weights
    e^8 above the others' and the likelihood's spread 4 nats."""
    from dust_amd import Context

    da, H = (1, 6) if model == "pendulum" else (2, 4)
    S = 8
    tm = ec.tie_members(tie, N) if tie else None
    sigma = ec.sigma_for(N)[0]
    lnorm = ec.log_norm(H, da, sigma)
    rng = np.random.default_rng(17 * N + H)
    theta, eps = _with_tie(ec.lattice_theta(N, H, da, N + 1, n_sat=2 if tm else 0), _eps(rng, 3, 1, S, N, H, da), tm)
    st, grid = STATE[model], _grid(model)
    w = None
    if tm:
        w = np.full(N, math.exp(-8.0), np.float32)
        w[list(tm)] = 1.0
    # probe: the costs tick 2 will see (its particles are tick 1's rolled ones), for the alpha that gives the case its spread
    base = dict(model=model, N=N, S=S, M=1, H=H, kernel="K1", lr=0.0, sigma_a=SIGMA_A, sigma_p=sigma, weighted_prior=wp, roll_strategy=strategy, seed=3)
    probe = Context(alpha=1.0, grid=grid, **base)
    probe.set_theta(theta)
    costs = probe.likelihood_sample_at(st, ec.roll(theta, -1, strategy).astype(np.float32), eps[1, 0])
    probe.close()
    alpha = ec.alpha_for(costs, kind)
    c = Context(alpha=alpha, grid=grid, **base)
    c.set_theta(theta)
    c.set_prior(theta)
    c.set_a_mat(theta)
    _, pw1 = c.svmpc_tick(st, 1, eps[0])
    mix_prev = pw1
    if w is not None:
        c.svmpc_update_prior(w)
        mix_prev = w
    for t in (1, 2):
        pre, s0 = c.get_theta(), c.tick_stats()
        if t == 1:
            assert np.array_equal(pre[:, :-1], ec.roll(theta, -1, strategy)[:, :-1])
        assert ec.min_separation(pre, sigma, sample=256) >= 40.0
        a_seq, pw = c.svmpc_tick(st, 1, eps[t])
        s1 = c.tick_stats()
        assert s1["tick2"] == s0["tick2"] + 1 and s1["replayed"] == s0["replayed"], (s0, s1)
        ll, lp = c.get_log_weights()
        note = "tick2 %s N=%d tick %d" % (model, N, t + 1)
        _check_weights(ll, lp, pw, a_seq, pre, kind if t == 1 else None, tm if t == 1 else None, note)
        _check_logmix_seen(lp, lnorm, mix_prev, wp, note)
        post, want = c.get_theta(), ec.roll(pre, -1, strategy)
        assert np.array_equal(post[:, :-1], want[:, :-1]) and np.abs(post - want).max() <= (ec.tol_mean(pre) if strategy == "mean" else 0.0), note
        means, probs = c.get_prior()
        assert np.array_equal(means, post)
        _check_probs(probs, pw, wp, note)
        mix_prev = pw
    c.close()


# ================================================================================================ the batched tick
BATCH_RUNS = [(m, N, wp, st, None) for m, st in (("pendulum", "repeat"), ("particle", "mean")) for N in ec.BATCH_N for wp in (False, True)]
BATCH_RUNS += [("pendulum", N, False, "repeat", t) for N, t in ((2, "d"), (63, "a"), (64, "d"))]


@pytest.mark.parametrize("model,N,wp,strategy,tie", BATCH_RUNS)
def test_batch_tail(model, N, wp, strategy, tie):
    """svmpc_batch.hpp's epilogue, B = 3 with a different spread per environment - flat, the subject (peaked; or the tie, in this
    environment only), flat with other weights: the first forward (displaced means: the spreads of the case table), then a second
    tick whose log_p shows the logmix the first one wrote."""
    from dust_amd import Context, _lib as L

    da, H = (1, 6) if model == "pendulum" else (2, 4)
    S, B = 8, 3
    tm = ec.tie_members(tie, N) if tie else None
    sigma = ec.sigma_for(N)[0]
    lnorm = ec.log_norm(H, da, sigma)
    rng = np.random.default_rng(5 * N + H)
    kinds = ["flat", "flat" if (tm or N < 2) else "peaked", "flat"]
    th, mu, w, ep = [], [], [], []
    for b in range(B):
        tb = tm if b == 1 else None
        t_, e_ = _with_tie(ec.lattice_theta(N, H, da, N + b, n_sat=2 if tb else 0), _eps(rng, 2, S, N, H, da), tb)
        th.append(t_)
        ep.append(e_)
        mu.append(_displaced(t_, _gaps(N, kinds[b], 1000 + N + b, tb), sigma))
        wb = (rng.random(N) + 0.5).astype(np.float32)
        if tb:
            wb[tb[1]] = wb[tb[0]]
        w.append(wb)
    th, mu, w, ep = np.stack(th), np.stack(mu), np.stack(w), np.stack(ep)
    proto = Context(model=model, N=N, S=S, M=1, H=H, kernel="K1", lr=0.0, alpha=1e-4 if da == 1 else 1e-7, sigma_a=SIGMA_A, sigma_p=sigma,
                    weighted_prior=wp, roll_strategy=strategy, grid=_grid(model), seed=3)
    bt = proto.svmpc_batch(B)
    bt.set(L.SVB_THETA, th)
    bt.set(L.SVB_PRIOR_MEANS, mu)
    bt.set(L.SVB_PRIOR_MIX, w)
    bt.set(L.SVB_A_MAT, th)
    states = np.stack([STATE[model]] * B)
    mix_prev, pre = w, th
    for t in (0, 1):
        bt.optimize(states, 1, ep[:, t:t + 1])
        assert np.array_equal(bt.get(L.SVB_THETA), pre)
        ll = bt.get(L.SVB_LOG_L)
        a_seq, pw = bt.forward()
        lp, post = bt.get(L.SVB_LOG_P), bt.get(L.SVB_THETA)
        mixw = bt.get(L.SVB_PRIOR_MIX).astype(np.float64)
        for b in range(B):
            note = "batch %s N=%d env %d tick %d" % (model, N, b, t + 1)
            first = t == 0
            _check_weights(ll[b], lp[b], pw[b], a_seq[b], pre[b], kinds[b] if first else None, tm if (first and b == 1) else None, note)
            if first:
                q = ((pre[b].astype(np.float64) - mu[b]) ** 2).sum((1, 2)) / (2.0 * sigma * sigma)
                want = ec.mixture(w[b], True)[1] - q
                tol = ec.tol_logmix(w[b]) + ec.tol_logmix_seen(lp[b], lnorm) + 4 * ec.EPS32 * q.max() + ec.sp(np.abs(want).max())
                assert np.abs(lp[b].astype(np.float64) - lnorm - want).max() <= tol, note
            else:
                _check_logmix_seen(lp[b], lnorm, mix_prev[b], wp, note)
            want = ec.roll(pre[b], -1, strategy)
            assert np.array_equal(post[b][:, :-1], want[:, :-1]), note
            assert np.abs(post[b] - want).max() <= (ec.tol_mean(pre[b]) if strategy == "mean" else 0.0), note
            _check_probs((mixw[b] / mixw[b].sum()).astype(np.float32), pw[b], wp, note)
        assert np.array_equal(bt.get(L.SVB_PRIOR_MEANS), post)
        mix_prev, pre = pw, post
    bt.close()
    # set(PRIOR_MIX): svmpc_batch_logmix_kernel, seen through LOG_P of the next forward on separated means
    vecs = _weight_vectors(N, rng)
    names = [k for k in ("zeros", "one_hot", "decades12") if k in vecs]
    while len(names) < B:
        names.append("decades12")
    wv = np.stack([vecs[k] for k in names])
    bt = proto.svmpc_batch(B)
    bt.set(L.SVB_THETA, th)
    bt.set(L.SVB_PRIOR_MEANS, th)
    bt.set(L.SVB_A_MAT, th)
    bt.set(L.SVB_PRIOR_MIX, wv)
    bt.optimize(states, 1, ep[:, :1])
    bt.forward()
    lp = bt.get(L.SVB_LOG_P)
    for b in range(B):
        _check_logmix_seen(lp[b], lnorm, wv[b], True, "batch set(PRIOR_MIX) %s N=%d" % (names[b], N))
    bt.close()
    proto.close()
