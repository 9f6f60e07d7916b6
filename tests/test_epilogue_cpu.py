"""The tick epilogue's float64 restatement (tests/epilogue_cases.py) without a device: pinned against torch in float64, against the
reference's recorded numbers (tests/golden), the C oracle held to it at every case size, the stated conditions of the case table and
its POWER - an fp32 emulation in three summation orders stays within half of every tolerance, every listed wrong variant is caught by
a named case (or is shown to be unobservable: see the module docstring of epilogue_cases)."""
import numpy as np
import pytest
import torch

import epilogue_cases as ec
from helpers import relerr
from test_oracle_golden import SVMPC_CASES

CASES = ec.weight_cases()
IDS = [c["id"] for c in CASES]
F64EPS = float(np.finfo(np.float64).eps)


def _case_inputs(c):
    return ec.synth_log_weights(c["N"], "flat" if c["kind"].startswith("tie") else c["kind"], c["seed"], c["tie"])


# ------------------------------------------------------------------------------------------------ the restatement against torch
@pytest.mark.parametrize("c", CASES, ids=IDS)
def test_weights_and_mixture_vs_torch_float64(c):
    ll, lp = _case_inputs(c)
    p, i_star, lse = ec.weights(ll, lp)
    lw = torch.as_tensor((ll + lp).astype(np.float64))
    tp = torch.softmax(lw, 0)
    assert np.abs(p - tp.numpy()).max() <= 1e-12 and abs(lse - float(torch.logsumexp(lw, 0))) <= 1e-12 * abs(lse)
    assert i_star == int(torch.argmax(tp))
    if c["tie"] is not None:
        assert i_star == c["tie"][0]
    for w in (p, np.ones_like(p)):
        # float64 tensors: Categorical clamps with the float64 eps
        cat = torch.distributions.Categorical(probs=torch.as_tensor(w))
        want = torch.log_softmax(cat.logits, -1).numpy()
        probs, lmx = ec.mixture(w, True, eps=F64EPS)
        assert np.abs(probs - cat.probs.numpy()).max() <= 1e-12
        assert np.abs(lmx - want).max() <= 1e-12 * max(1.0, np.abs(want).max())
    # float32 tensors, as the reference holds them: the clamp is the float32 eps; torch's own fp32 arithmetic is within the tolerance
    w32 = p.astype(np.float32)
    cat = torch.distributions.Categorical(probs=torch.as_tensor(w32))
    want = torch.log_softmax(cat.logits, -1).numpy().astype(np.float64)
    assert np.abs(ec.mixture(w32, True)[1] - want).max() <= ec.tol_logmix(w32)


@pytest.mark.parametrize("N", [n for n in sorted(set(ec.FINALIZE_N + ec.TICK2_N + ec.BATCH_N)) if n <= 1025])
def test_prior_log_prob_vs_torch_float64(N):
    """(O(N^2): the sizes up to 1025)"""
    D = torch.distributions
    rng = np.random.default_rng(N)
    H, da = 3, 2
    th, mu = rng.standard_normal((N, H, da)), rng.standard_normal((N, H, da))
    sig = np.array([0.7, 1.9])
    _, lmx = ec.mixture(rng.random(N) + 0.01, True, eps=F64EPS)
    mix = D.Categorical(probs=torch.as_tensor(np.exp(lmx)))
    comp = D.Independent(D.MultivariateNormal(torch.as_tensor(mu), covariance_matrix=torch.diag(torch.as_tensor(sig ** 2))), 1)
    want = D.MixtureSameFamily(mix, comp).log_prob(torch.as_tensor(th)).numpy()
    got = ec.prior_log_prob(th, mu, lmx, sig)
    assert np.abs(got - want).max() <= 1e-12 * max(1.0, np.abs(want).max())
    assert abs(ec.log_norm(H, da, sig) - float(comp.log_prob(torch.as_tensor(mu))[0])) <= 1e-12 * 10


@pytest.mark.parametrize("model,da,H", ec.ROLL_SHAPES)
def test_roll_vs_torch_float64(model, da, H):
    th32, last = ec.roll_inputs(7, H, da, 10 * H + da)
    t0 = torch.as_tensor(th32.astype(np.float64))
    for steps in ec.roll_steps(H):
        for strategy in ec.STRATEGIES:
            t = t0.roll(steps, dims=-2)
            if strategy == "repeat":
                t[..., -1, :] = t[..., -2, :]
            elif strategy == "resample":
                t[..., -1, :] = torch.as_tensor(last.astype(np.float64))
            else:
                t[..., -1, :] = t.mean(dim=-2)
            got = ec.roll(th32, steps, strategy, last)
            assert np.abs(got - t.numpy()).max() <= 1e-12, (steps, strategy)


def test_roll_h1_follows_the_reference():
    th = np.arange(6, dtype=np.float32).reshape(3, 1, 2)
    assert np.array_equal(ec.roll(th, -1, "mean"), th)
    with pytest.raises(IndexError):
        ec.roll(th, -1, "repeat")
    with pytest.raises(IndexError):
        t = torch.as_tensor(th).roll(-1, dims=-2)
        t[..., -1, :] = t[..., -2, :]


# ------------------------------------------------------------------------------------------------ ... against the reference's numbers
@pytest.mark.parametrize("name", SVMPC_CASES)
def test_restatement_vs_recorded_ticks(golden, name):
    """tolerances: those of test_oracle_golden.test_forward for the same fields"""
    g = golden(name)
    need = ("tick_log_l", "tick_log_p", "tick_p_weights", "tick_a_seq", "tick_theta_rolled", "tick_prior_probs")
    assert all(k in g for k in need), name
    T, K = g["eps"].shape[:2]
    wp, strategy = bool(int(g["weighted_prior"])), str(g["roll_strategy"])
    for t in range(T):
        p, i_star, _ = ec.weights(g["tick_log_l"][t], g["tick_log_p"][t])
        assert i_star == int(np.argmax(g["tick_p_weights"][t]))
        assert relerr(p, g["tick_p_weights"][t]) < 2e-3
        th = g["theta_after"][t, K - 1]
        assert np.array_equal(th[i_star], g["tick_a_seq"][t])
        assert relerr(ec.roll(th, -1, strategy), g["tick_theta_rolled"][t]) < 1e-6
        assert relerr(ec.mixture(g["tick_p_weights"][t], wp)[0], g["tick_prior_probs"][t]) < 2e-3


def test_restatement_vs_recorded_disco_step(golden):
    g = golden("disco_mppi")
    for strat in ("argmax", "average"):
        nxt, a_seq, am = ec.disco_step(g["a_mat1"], g["a_mix"], strat, 2, -2.0, 2.0)
        assert relerr(nxt, g["step_%s_actions" % strat]) < 1e-6
        assert relerr(a_seq, g["step_%s_a_seq" % strat]) < 1e-6
        assert relerr(am, g["step_%s_a_mat" % strat]) < 1e-6
    nxt, a_seq, _ = ec.disco_step(g["a_mat1"], g["a_mix"], "external", 1, -2.0, 2.0, ext=g["step_external_in"])
    assert np.array_equal(nxt, g["step_external_actions"]) and np.array_equal(a_seq, g["step_external_a_seq"])
    assert abs(float(np.asarray(g["a_mix"], np.float64).sum()) - 1.0) < 1e-4 * 4  # (the recorded a_mix is a softmax: test_disco_mppi's 1e-4)


# ------------------------------------------------------------------------------------------------ the C oracle
ORACLE_N = sorted(set(ec.FINALIZE_N + ec.TICK2_N + ec.BATCH_N))


@pytest.mark.parametrize("N", ORACLE_N)
def test_oracle_forward_vs_restatement(N):
    """orc_forward at every case size, both values of weighted_prior, every roll= it takes: p against the restatement fed the oracle's
    own log_l / log_p (tol_p), first-index argmax on an exact tie, a_seq a copy, the roll, the refreshed prior.  roll=RESAMPLE is not
    implemented by orc_forward: it PINS what it computes, the `repeat` result (the device takes the resampled row from the caller).
    (O(N^2): from 4 095 on one configuration per spread, from 16 383 on the flat spread only.)"""
    import oracle
    from oracle import Oracle, grid_4x4_map

    big = N > 2049
    for da, model in ((1, "pendulum"), (2, "particle")):
        if big and da == 2:
            continue
        H, S = 3, 2
        rng = np.random.default_rng(7 * N + da)
        o = Oracle(model=model, N=N, S=S, M=1, H=H, grid=grid_4x4_map() if da == 2 else None)
        th, _ = ec.roll_inputs(N, H, da, N + da)
        if N >= 4:  # an exact tie of the best particle: equal costs, the prior means far apart (log_p = log mix + const for every row)
            i, j = ec.tie_members("d", N) if N < 70 else ec.tie_members("b", N)
        mu = th + 200.0 * np.arange(N, dtype=np.float32)[:, None, None]
        th = mu.copy()
        sig = np.array([1.5, 0.75], np.float32)[:da]
        for kind in ("flat", "peaked"):
            costs = (rng.random((S, N)) * (8.0 if kind == "flat" else 400.0) + 50.0).astype(np.float32)
            if kind == "flat" and N >= 4:
                costs[:, [i, j]] = 40.0
            for wp in ((False, True) if not big else (True,)):
                for rs, rname in ((oracle.ROLL_REPEAT, "repeat"), (oracle.ROLL_MEAN, "mean"), (2, "repeat")):  # (2: the library's DUST_ROLL_RESAMPLE)
                    if big and rs != oracle.ROLL_MEAN:
                        continue
                    r = o.forward(costs, th, mu, np.ones(N, np.float32), sig, 1.0, weighted_prior=wp, roll=rs)
                    p, i_star, _ = ec.weights(r["log_l"], r["log_p"])
                    lw = r["log_l"] + r["log_p"]
                    assert ec.p_ok(r["p_weights"], p, ec.tol_p(lw)), (kind, wp, rname, ec.p_err(r["p_weights"], p), ec.tol_p(lw))
                    assert r["i_star"] == i_star and np.array_equal(r["a_seq"], th[i_star])
                    if kind == "flat" and N >= 4:
                        assert lw[i] == lw[j] == lw.max() and i_star == i
                    want = ec.roll(th, -1, rname)
                    if rname == "mean":
                        assert np.array_equal(r["theta"][:, :-1], want[:, :-1])
                        assert np.abs(r["theta"] - want).max() <= ec.tol_mean(th)
                    else:
                        assert np.array_equal(r["theta"], want)
                    assert np.array_equal(r["mu"], r["theta"])
                    assert np.array_equal(r["mix"], r["p_weights"] if wp else np.ones(N, np.float32))
                    lmx = o.log_mix(r["mix"])
                    assert np.abs(lmx - ec.mixture(r["mix"], True)[1]).max() <= ec.tol_logmix(r["mix"]), (kind, wp)
        if N <= 1025:  # log_p itself, with a mixture that is not uniform and means that overlap
            mu2 = (th + rng.standard_normal(th.shape)).astype(np.float32)
            w = (rng.random(N) + 0.01).astype(np.float32)
            r = o.forward(costs, th, mu2, w, sig, 1.0)
            want = ec.prior_log_prob(th, mu2, ec.mixture(w, True)[1], sig)
            assert np.abs(r["log_p"] - want).max() <= 1e-5 * np.abs(want).max()


@pytest.mark.parametrize("N,da", ec.DISCO_SHAPES)
def test_oracle_disco_step_vs_restatement(N, da):
    from oracle import Oracle, grid_4x4_map

    H = ec.DISCO_H
    o = Oracle(model="pendulum" if da == 1 else "particle", N=N, S=1, M=1, H=H, grid=grid_4x4_map() if da == 2 else None)
    tie = ec.tie_members("b", N) or ec.tie_members("d", N)
    am, w, ext, lo, hi = ec.disco_inputs(N, H, da, 3 * N + da, tie)
    for steps in (1, 2, H):
        for strat in ("argmax", "average", "external"):
            nxt, a_seq, am1 = o.disco_step(am, w, strat, steps, lo, hi, ext)
            wn, ws, wa = ec.disco_step(am, w, strat, steps, lo, hi, ext)
            if strat == "average":
                tol = np.roll(ec.tol_average(am, w), -steps, axis=0)
                assert (np.abs(a_seq - ws) <= tol + 1e-300).all() and (np.abs(nxt - wn) <= ec.tol_average(am, w)[:steps]).all()
            else:
                assert np.array_equal(nxt, wn) and np.array_equal(a_seq, ws)
            assert np.array_equal(am1, wa), (steps, strat)
    if tie:
        assert w[tie[0]] == w[tie[1]] == w.max()
        assert np.array_equal(o.disco_step(am, w, "argmax", 1, lo, hi)[0], np.clip(am[tie[0], :1], lo, hi))


# ------------------------------------------------------------------------------------------------ the stated conditions
@pytest.mark.parametrize("c", CASES, ids=IDS)
def test_case_conditions(c):
    ll, lp = _case_inputs(c)
    p, i_star, _ = ec.weights(ll, lp)
    if c["kind"] == "flat":
        assert (p >= ec.P_FLOOR).all()
    elif c["kind"] == "peaked":
        probs = ec.mixture(p.astype(np.float32), True)[0]
        assert probs.max() >= 1.0 - ec.EPS32 and probs.min() <= ec.EPS32
        assert (p < ec.P_FLOOR).any() or c["N"] < 8
    else:
        i, j = c["tie"]
        lw = ll + lp
        assert i < j < c["N"] and lw[i] == lw[j] == lw.max() and int((lw == lw.max()).sum()) == 2 and i_star == i
        (ri, wi, li), (rj, wj, lj) = ec.place(i), ec.place(j)
        if c["kind"] == "tie_a":
            assert (ri, wi) == (rj, wj) and li != lj
        elif c["kind"] == "tie_b":
            assert ri == rj and wi != wj
        elif c["kind"] == "tie_c":
            assert ri != rj and (wi, li) == (wj, lj)
        else:
            assert (i, j) == (0, c["N"] - 1)


def test_tie_cases_cover_waves_and_register_rows():
    kinds = {(c["kind"], c["N"]) for c in CASES}
    for N in ec.FINALIZE_N:
        assert ("tie_d", N) in kinds or N < 2
        assert ("tie_b", N) in kinds or N <= 66
        assert ("tie_c", N) in kinds or N <= ec.LANES
        assert ("tie_a", N) in kinds or N < 4


# ------------------------------------------------------------------------------------------------ power
_caught = {}


def _note(variant, case_id):
    _caught.setdefault(variant, []).append(case_id)


@pytest.mark.parametrize("c", CASES, ids=IDS)
def test_power_weights_and_mixture(c):
    ll, lp = _case_inputs(c)
    lw = ll + lp
    p, i_star, _ = ec.weights(ll, lp)
    tp = ec.tol_p(lw)
    for wp in (False, True):
        for order in ec.ORDERS:
            e = ec.epilogue32(ll, lp, wp, order)
            rel, ab = ec.p_err(e["p"], p)
            assert rel <= tp / 2 and ab <= ec.P_FLOOR / 2, (order, rel, tp)
            assert abs(float(e["p"].astype(np.float64).sum()) - 1.0) <= tp / 2
            assert e["i_star"] == i_star
            _, lmx = ec.mixture(e["mixw"], wp)
            tl = ec.tol_logmix(e["mixw"], wp)
            assert np.abs(e["logmix"] - lmx).max() <= tl / 2, (order, wp, np.abs(e["logmix"] - lmx).max(), tl)
        good = ec.epilogue32(ll, lp, wp)
        probs, lmx = ec.mixture(good["mixw"], wp)
        tl = ec.tol_logmix(good["mixw"], wp)
        for v in ec.WEIGHT_VARIANTS:
            bad = ec.epilogue32(ll, lp, wp, variant=v)
            if v in ("tie_last", "argmax_lw"):
                if bad["i_star"] != i_star:
                    _note(v, c["id"])
            elif v == "mixw_from_lw":
                seen = probs > 0
                if wp and np.abs(bad["probs"][seen] / probs[seen] - 1.0).max() > 2 * (tp + 2 * ec.EPS32):
                    _note(v, c["id"])
            else:
                with np.errstate(invalid="ignore"):
                    dev = np.abs(bad["logmix"].astype(np.float64) - lmx)
                    dev = float(np.where(np.isnan(dev), np.inf, dev).max())
                if v == "no_upper_clamp":
                    assert dev <= tl / 2 + 2 * ec.EPS32, "unobservable by construction (module docstring of epilogue_cases)"
                if dev > 2 * tl:
                    _note(v, c["id"])


@pytest.mark.parametrize("model,da,H", ec.ROLL_SHAPES)
def test_power_roll(model, da, H):
    th, last = ec.roll_inputs(7, H, da, 10 * H + da)
    tm = ec.tol_mean(th)
    for steps in ec.roll_steps(H):
        for strategy in ec.STRATEGIES:
            want = ec.roll(th, steps, strategy, last)
            for order in ec.ORDERS:
                got = ec.roll32(th, steps, strategy, last, order)
                if strategy == "mean":
                    assert np.array_equal(got[:, :-1], want[:, :-1]) and np.abs(got - want).max() <= tm / 2
                else:
                    assert np.array_equal(got, want)
            for v in ec.ROLL_VARIANTS:
                bad = ec.roll32(th, steps, strategy, last, variant=v)
                miss = (np.abs(bad - want).max() > 2 * tm) if strategy == "mean" else (not np.array_equal(bad, want))
                if miss:
                    _note(v, "%s-H%d-steps%d-%s" % (model, H, steps, strategy))


@pytest.mark.parametrize("N,da", ec.DISCO_SHAPES)
def test_power_disco(N, da):
    H = ec.DISCO_H
    tie = ec.tie_members("b", N) or ec.tie_members("d", N)
    am, w, ext, lo, hi = ec.disco_inputs(N, H, da, 3 * N + da, tie)
    assert (np.abs(am[int(np.argmax(w))]) > hi).any(), "the chosen row must have entries the bounds clamp"
    for steps in (1, 2, H):
        for strat in ("argmax", "average", "external"):
            wn, ws, wa = ec.disco_step(am, w, strat, steps, lo, hi, ext)
            gn, gs, ga = ec.disco32(am, w, strat, steps, lo, hi, ext)
            assert np.array_equal(ga, wa) and np.abs(gs - ws).max() <= (ec.tol_average(am, w).max() / 2 if strat == "average" else 0)
            for v in ec.DISCO_VARIANTS:
                if not np.array_equal(ec.disco32(am, w, strat, steps, lo, hi, ext, variant=v)[2], wa):
                    _note(v, "N%d-da%d-steps%d-%s" % (N, da, steps, strat))


def test_power_every_variant_is_caught_by_a_named_case():
    """(runs after the power tests of this module, which fill the record)"""
    need =[v for v in ec.WEIGHT_VARIANTS + ec.ROLL_VARIANTS + ec.DISCO_VARIANTS if v not in ("argmax_lw", "no_upper_clamp")]
    if not all(v in _caught for v in need):  # selected alone: run the power tests here
        for c in CASES:
            test_power_weights_and_mixture(c)
        for s in ec.ROLL_SHAPES:
            test_power_roll(*s)
        for s in ec.DISCO_SHAPES:
            test_power_disco(*s)
    missing = [v for v in need if v not in _caught]
    assert not missing, "no case catches: %s" % missing
    assert "argmax_lw" not in _caught, "documented as never differing: %s" % _caught.get("argmax_lw")
    assert "no_upper_clamp" not in _caught
    assert any(i.startswith("tie_") for i in _caught["tie_last"])
    assert all(int(i[6:]) >= 1020 for i in _caught["no_log_softmax"]), _caught["no_log_softmax"]
    assert any("particle" in i or "skid" in i for i in _caught["mean_all_D"])
