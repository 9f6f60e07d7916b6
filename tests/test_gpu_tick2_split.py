"""The prior pass of the one-launch tick (dust_amd/csrc/tick2.hpp t2_prior_pass_w) at the shapes where a cut of its key steps meets an
edge.  Written for a form that handed the last live steps of every unit to the rollout waves (measured slower and not kept: DESIGN.md
section 4, profiles/tick2_phase1_share.txt); what it pins holds for any schedule of the pass - wave priorities, another cut of the
steps - and the other files do not cover it: N = 1024 (no masked key) and N = 1000 (masked keys in the last live step), N = 896 and 512
(the live steps end inside / in front of the padded ones), N = 768 with IMQ, N = 64 (one live step), one iteration per tick (the go
word is picked up in front of barrier B1), Particle with sampled dynamics at N = 512 / 1024, the general rollout form (`bad`) in front
of the pass, served (armed) ticks at masked shapes, and grad_pri / log p of a cfg2 tick against the CPU oracle - where a key step
counted twice or dropped shows as an error of the order of 1 / steps, not as rounding.  References: the launch-per-iteration paths
(DUST_NO_TICK2) one tick at a time - the take-over scheme and the tolerances of test_gpu_tick2.test_tick2_equals_launch_per_iteration -
and the oracle at test_tick2_stage_parity_vs_oracle's bound.  Shown once by a mutation that is not committed (the pass starting at its
third step): all 23 cases fail."""
import numpy as np
import pytest

from helpers import elemerr
from test_gpu_tick2 import TOL, _make, _make_with_env, _snapshot, _state

pytestmark = pytest.mark.gpu

SHAPES = [
    # model, N, S, H, iters, M, kw                                 live wide steps (128 keys each) of the 8 a unit runs
    ("pendulum", 1024, 128, 30, 3, 1, {}),                         # 8, no masked key
    ("pendulum", 1000, 128, 30, 2, 1, {}),                         # 8, masked keys in the last one
    ("pendulum", 896, 64, 30, 2, 1, {}),                           # 7: the last step is padding
    ("pendulum", 512, 64, 30, 2, 1, {}),                           # 4
    ("pendulum", 64, 128, 15, 2, 1, {}),                           # 1
    ("pendulum", 1024, 64, 30, 1, 1, {}),                          # ONE iteration: the go word is picked up in front of barrier B1
    ("pendulum", 768, 64, 24, 2, 1, dict(kernel="IMQ")),           # 6
    ("particle", 512, 64, 16, 2, 4, dict(kernel="IMQ")),           # sampled dynamics (M > 1): the general rollout in front of barrier B1
    ("particle", 1024, 64, 12, 2, 2, {}),
]


@pytest.mark.parametrize("ext_noise", [True, False])
@pytest.mark.parametrize("model,N,S,H,iters,M,kw", SHAPES)
def test_split_tick_equals_launch_per_iteration(model, N, S, H, iters, M, kw, ext_noise):
    """Two contexts side by side, three ticks, the launch-per-iteration context taking the one-launch context's state over after every
    tick (test_tick2_equals_launch_per_iteration's scheme and tolerances), at the shapes where a cut of the key steps meets an edge."""
    a, rng_a = _make_with_env({}, model, N, S, H, M=M, **kw)
    b, _ = _make_with_env({"DUST_NO_TICK2": "1"}, model, N, S, H, M=M, **kw)
    da = 1 if model == "pendulum" else 2
    st = _state(model)
    for t in range(3):
        eps = rng_a.standard_normal((iters, S, N, H, da)).astype(np.float32) if ext_noise else None
        params = None
        if M > 1:
            params = (1.0 + 0.1 * rng_a.standard_normal((iters, M, 1 if model == "particle" else 2))).astype(np.float32)
        ra = a.svmpc_tick(st, iters, eps=eps, params=params)
        rb = b.svmpc_tick(st, iters, eps=eps, params=params)
        sa, sb = dict(a_seq=ra[0], pw=ra[1], **_snapshot(a)), dict(a_seq=rb[0], pw=rb[1], **_snapshot(b))
        for k in ("costs", "score", "phi", "theta", "a_mat", "ll", "lp", "a_seq"):
            tol = TOL * (25 if k in ("score", "phi", "theta", "a_mat", "a_seq", "ll") else 1)
            err = elemerr(sa[k], sb[k])
            print("tick %d %-6s elemerr %.3g (tol %.3g)" % (t, k, err, tol))
            assert err < tol, (t, k, err)
        print("tick %d pw     max abs %.3g" % (t, np.abs(sa["pw"] - sb["pw"]).max()))
        assert np.abs(sa["pw"] - sb["pw"]).max() < 2e-3, t
        b.set_theta(a.get_theta())
        b.set_a_mat(a.get_a_mat())
    stats_a, stats_b = a.tick_stats(), b.tick_stats()
    a.close()
    b.close()
    assert stats_a["tick2"] == 2 and stats_a["replayed"] == 0, stats_a
    assert stats_b["tick2"] == 0, stats_b


def test_split_with_non_finite_noise_of_one_particle():
    """Caller-supplied noise with one non-finite entry: the rollout waves of that particle leave the fast rollout form (`bad`).  One
    iteration is stage-local: the costs - finite or not in the same places - and the WHOLE prior score, which depends on the particles
    only, must agree with the launch-per-iteration path."""
    model, N, S, H = "pendulum", 1000, 128, 30
    n_bad = 517
    res = []
    for env in ({}, {"DUST_NO_TICK2": "1"}):
        c, rng = _make_with_env(env, model, N, S, H)
        st = _state(model)
        c.svmpc_tick(st, 1, eps=rng.standard_normal((1, S, N, H, 1)).astype(np.float32))  # aliases the prior
        eps = rng.standard_normal((1, S, N, H, 1)).astype(np.float32)
        eps[0, 5, n_bad, 3, 0] = np.inf
        before = c.tick_stats()["tick2"]
        c.svmpc_optimize(st, 1, eps=eps)
        res.append((c.get_costs(), c.get_score_parts()[1], c.tick_stats()["tick2"] - before, c.tick_stats()["replayed"]))
        c.close()
    (c0, g0, n0, r0), (c1, g1, n1, r1) = res
    assert n0 == 1 and r0 == 0 and n1 == 0, (n0, r0, n1)
    fin = np.isfinite(c0)
    assert np.array_equal(fin, np.isfinite(c1)) and np.isfinite(g0).all() and np.isfinite(g1).all()
    print("costs elemerr %.3g  grad_pri elemerr %.3g" % (elemerr(c0[fin], c1[fin]), elemerr(g0, g1)))
    assert elemerr(c0[fin], c1[fin]) < TOL
    assert elemerr(g0, g1) < 25 * TOL


@pytest.mark.parametrize("N,S,iters", [(1000, 128, 3), (512, 64, 1)])
def test_split_served_ticks_are_bit_identical(N, S, iters):
    """In iteration 0 of an armed launch the rollout waves wait for the plant state while the pair waves run the pass: whatever the
    schedule of the pass, a served loop is the unserved one bit for bit (test_gpu_serve's comparison) - here at a masked shape and
    at a half-padded one with one iteration per tick."""
    from test_gpu_serve import _loop

    a, _ = _make("pendulum", N, S, 30)
    ra, tha, ama, ca, sa = _loop(a, "pendulum", iters, 12, serve=False)
    a.close()
    b, _ = _make("pendulum", N, S, 30)
    rb, thb, amb, cb, sb = _loop(b, "pendulum", iters, 12, serve=True)
    b.close()
    for t, ((a0, p0, s0), (a1, p1, s1)) in enumerate(zip(ra, rb)):
        assert np.array_equal(s0, s1), t
        assert np.array_equal(a0, a1), (t, np.abs(a0 - a1).max())
        assert np.array_equal(p0, p1), t
    assert np.array_equal(tha, thb) and np.array_equal(ama, amb) and np.array_equal(ca, cb)
    assert sa["served"] == 0 and sa["replayed"] == 0
    assert sb["served"] == 12 and sb["replayed"] == 0, sb


@pytest.mark.parametrize("N", [1024, 1000])
def test_split_prior_score_and_log_density_vs_oracle(N):
    """grad_pri and log p of one tick at the shape bench.py times (and its masked neighbour) against the CPU oracle, at the bound of
    test_tick2_stage_parity_vs_oracle (1e-5 element-wise): a key step counted twice or dropped at the seam is an error of the order of
    1 / steps, not rounding."""
    from oracle import Oracle

    S, H, sig, alpha = 128, 30, 2.0, 1.0
    st = _state("pendulum")
    # two contexts from one start: the first stops behind the iteration (particles before the roll, stage outputs), the second runs the
    # whole tick, i.e. the log-density pass inside the one-launch kernel
    c, rng = _make("pendulum", N, S, H)
    d, _ = _make("pendulum", N, S, H)
    eps0 = rng.standard_normal((1, S, N, H, 1)).astype(np.float32)
    eps = rng.standard_normal((1, S, N, H, 1)).astype(np.float32)
    for x in (c, d):
        x.svmpc_tick(st, 1, eps=eps0)  # aliases the prior
    th, (mu1, mix) = c.get_theta(), c.get_prior()
    assert np.array_equal(mu1, th) and np.array_equal(d.get_theta(), th)
    before = c.tick_stats()["tick2"], d.tick_stats()["tick2"]
    c.svmpc_optimize(st, 1, eps=eps)
    costs, (gl, gp), th1 = c.get_costs(), c.get_score_parts(), c.get_theta()
    d.svmpc_tick(st, 1, eps=eps)
    ll, lp = d.get_log_weights()
    assert c.tick_stats()["tick2"] == before[0] + 1 and d.tick_stats()["tick2"] == before[1] + 1, (c.tick_stats(), d.tick_stats())
    assert c.tick_stats()["replayed"] == 0 and d.tick_stats()["replayed"] == 0
    assert np.array_equal(d.get_costs(), costs)
    c.close()
    d.close()
    o = Oracle(model="pendulum", N=N, S=S, M=1, H=H)
    sv = np.full(1, sig, np.float32)
    actions = o.sample_actions(th, eps[0], sv)
    _, gp_ref, _ = o.score(th, th, mix, sv, costs, actions, alpha, sv)
    f = o.forward(costs, th1, th1, mix, sv, alpha)  # the prior means alias the updated particles (svgd.py:87)
    print("N %d grad_pri elemerr %.3g  log p elemerr %.3g" % (N, elemerr(gp, gp_ref), elemerr(lp, f["log_p"])))
    assert elemerr(gp, gp_ref) < 1e-5, elemerr(gp, gp_ref)
    assert elemerr(lp, f["log_p"]) < 1e-5, elemerr(lp, f["log_p"])
