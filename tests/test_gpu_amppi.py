"""AMPPI on the device (dust_amppi_update / dust_amd.controllers.AMPPI) against the reference's own `AMPPI.update_actions`
(tests/golden/amppi_*.npz from tests/golden/make_golden_amppi.py; scenarios in tests/amppi_cases.py).  Every bound is the fixture's
stored tolerance - max(1e-5, 2 x the reference's own fp32 error), capped at 5e-5 by the generator."""
import copy

import numpy as np
import pytest
import torch

import amppi_cases as cases
from helpers import elemerr

pytestmark = pytest.mark.gpu

VARIANTS = ("costs_disco", "costs_noctrl", "costs_single", "costs_mean")


def _err(got, g, q):
    """elemerr against the reference's fp32 or float64 value of quantity q, whichever is nearer"""
    return min(elemerr(got, g[q]), elemerr(got, cases.twin(g, q)))


def _ctx(s, g=None, **kw):
    from dust_amd import Context
    from oracle import grid_4x4_map

    c = Context(grid=grid_4x4_map() if s["family"] == "particle" else None, **cases.context_kwargs(s, **kw))
    if s["mode"] == "ut":
        c.set_param_weights(g["loc_weights"])
    return c


def _params(s, g):
    return g["sigma_points"] if s["mode"] == "ut" else g.get("params")


def _update(c, s, g, **kw):
    c.set_a_seq(g["a_seq0"])
    return c.amppi_update(g["state"], g["actions"], _params(s, g), shared_params=s["mode"] == "single", **kw)


@pytest.mark.parametrize("name", cases.NAMES)
def test_fixture_through_the_context(golden, name):
    """every fixture: costs, omega, the updated sequence and (where kept) the states at the stored tolerances - and NOT within
    tolerance of any power variant (instantaneous cost on t = 0 .. H - 1, no lambda term, row 0 for all, plain mean, no clamp)"""
    s, g = cases.BY_TAG[name], golden("amppi_" + name)
    c = _ctx(s, g)
    costs, omega, a_seq, states, acts = _update(c, s, g, want_states=s["states"], want_actions=True)
    errs = dict(costs=_err(costs, g, "costs"), omega=_err(omega, g, "omega"), a_seq1=_err(a_seq, g, "a_seq1"))
    if s["states"]:
        errs["states"] = _err(states, g, "states")
    print(name, " ".join("%s %.2e / %.1e" % (q, e, float(g["tol_" + q])) for q, e in errs.items()))
    for q, e in errs.items():
        assert e < float(g["tol_" + q]), (q, e, float(g["tol_" + q]))
    assert np.array_equal(acts, g["actions"]) and np.array_equal(c.get_a_seq(), a_seq) and np.array_equal(c.get_costs().reshape(-1), costs)
    for v in VARIANTS:
        if v in g:
            assert elemerr(costs, g[v]) > float(g["tol_costs"]), v
    if "a_seq1_noclamp" in g:
        assert elemerr(a_seq, g["a_seq1_noclamp"]) > float(g["tol_a_seq1"])
    if name == "pend_one":
        want = g["a_seq0"] + (g["actions"][0] - g["a_seq0"])  # (fp32: a + fl(b - a) need not be b)
        assert omega[0] == 0.0 and np.array_equal(a_seq, np.clip(want, np.float32(-2.0), np.float32(2.0)))
    c.close()


def _mirror(s, g):
    """the repo's own model and cost classes for scenario s -> (model, inst_cost_fn, term_cost_fn)"""
    from dust_amd.costs import PendulumQuadCos, QuadraticCost
    from dust_amd.models import CartPoleModel, Particle, PendulumModel, SkidSteerRobot

    f = cases.FAMILY[s["family"]]
    up = tuple(s["up"]) or None
    if s["family"] == "pendulum":
        cost = PendulumQuadCos(f["w_cos"], f["w_vel"])
        return PendulumModel(uncertain_params=up, **f["defaults"]), cost.inst_cost, cost.term_cost
    if s["family"] == "particle":
        m = Particle(**cases.PART_ENV, mass=f["defaults"]["mass"], uncertain_params=list(s["up"]) or None)
        return m, m.default_inst_cost, m.default_term_cost
    cost = QuadraticCost(f["goal"], f["w_state"], f["w_term"])
    if s["family"] == "cartpole":
        return CartPoleModel(dt=f["dt"], uncertain_params=up, **f["defaults"]), cost.inst_cost, cost.term_cost
    m = SkidSteerRobot(f["dt"], min_wheel_speed=torch.tensor(f["lo"]), max_wheel_speed=torch.tensor(f["hi"]), uncertain_params=up, **f["defaults"])
    return m, cost.inst_cost, cost.term_cost


def _controller(s, g, model, inst, term, **kw):
    from dust_amd.controllers import AMPPI
    from dust_amd.utils.utf import MerweScaledUTF

    f = cases.FAMILY[s["family"]]
    sampling = MerweScaledUTF(n=len(s["up"]), alpha=cases.UT_ALPHA) if s["mode"] == "ut" else s["mode"]
    return AMPPI(model.observation_space, model.action_space, s["H"], s["S"], lambda_=f["lam"], a_cov=torch.tensor(cases.a_cov_of(s)),
                 inst_cost_fn=inst, term_cost_fn=term, params_sampling=sampling, init_actions=torch.tensor(g["a_seq0"]), **kw)


def _feed(model, rows):
    model.sample_params = lambda n, r=rows: model.params_to_dict(torch.as_tensor(r)[:n])


@pytest.mark.parametrize("name", cases.CLASS_CASES)
def test_fixture_through_the_class(golden, name):
    """AMPPI.update_actions on the repo's own model classes: recorded rows through model.sample_params, sigma points from
    model.params_dist"""
    s, g = cases.BY_TAG[name], golden("amppi_" + name)
    model, inst, term = _mirror(s, g)
    ctrl = _controller(s, g, model, inst, term)
    assert ctrl.params_sampling is not None and np.array_equal(ctrl.a_seq.numpy(), g["a_seq0"])
    if "params" in g:
        _feed(model, g["params"])
    if s["mode"] == "ut":
        model.params_dist = torch.distributions.MultivariateNormal(torch.tensor(g["dist_mean"]), covariance_matrix=torch.diag(torch.tensor(g["dist_std"]) ** 2))
    costs, states, acts, omega = ctrl.update_actions(model, torch.tensor(g["state"]), torch.tensor(g["actions"]))
    pts = 2 * len(s["up"]) + 1 if s["mode"] == "ut" else 1
    assert tuple(states.shape) == (s["S"] * pts, s["H"] + 1, cases.FAMILY[s["family"]]["ds"]) and np.array_equal(acts.numpy(), g["actions"])
    assert _err(costs.numpy(), g, "costs") < float(g["tol_costs"])
    assert _err(omega.numpy(), g, "omega") < float(g["tol_omega"])
    assert _err(ctrl.a_seq.numpy(), g, "a_seq1") < float(g["tol_a_seq1"])
    if s["states"]:
        assert _err(states.numpy(), g, "states") < float(g["tol_states"])
    ctrl.return_rollouts = False
    ctrl.a_seq = torch.tensor(g["a_seq0"])
    costs2, states2, acts2, _ = ctrl.update_actions(model, torch.tensor(g["state"]), torch.tensor(g["actions"]))
    assert states2 is None and acts2 is None and np.array_equal(costs2.numpy(), costs.numpy())


def test_closed_loop_through_the_class(golden):
    """pend_loop: update_actions from recorded actions and rows, the plant's step with the first planned action, roll(1) - four ticks,
    each at its own tolerance"""
    s, g = cases.LOOP, golden("amppi_pend_loop")
    from dust_amd.models import PendulumModel

    model, inst, term = _mirror(s, g)
    plant = PendulumModel()
    ctrl = _controller(s, g, model, inst, term)
    ctrl.return_rollouts = False
    state = torch.tensor(g["state"])
    for k in range(s["ticks"]):
        _feed(model, g["params"][k])
        costs, _, _, omega = ctrl.update_actions(model, state, torch.tensor(g["actions"][k]))
        a_seq = ctrl.a_seq
        state = plant.step(state.view(1, -1), a_seq[0].view(1, -1)).view(-1)
        got = dict(costs=costs.numpy(), omega=omega.numpy(), a_seq1=a_seq.numpy(), plant=state.numpy())
        for q, v in got.items():
            e = min(elemerr(v, g[q][k]), elemerr(v, g[q + "_f64"][k]))
            assert e < float(g["tol_" + q][k]), (k, q, e)
        for v in ("costs_disco", "costs_noctrl", "costs_single"):
            assert elemerr(got["costs"], g[v][k]) > float(g["tol_costs"][k]), (k, v)
        ctrl.roll(1)
        rolled = ctrl.a_seq.numpy()
        assert np.array_equal(rolled[:-1], a_seq.numpy()[1:]) and not rolled[-1].any()
    ctrl.roll(s["H"] + 3)
    assert not ctrl.a_seq.numpy().any()


def test_many_workgroups_give_the_same_bits(golden):
    """pend_big_4099 (17 workgroups; whichever arrives last reduces) on two fresh contexts: bit-identical costs, omega and a_seq"""
    s, g = cases.BY_TAG["pend_big_4099"], golden("amppi_pend_big_4099")
    runs = []
    for _ in range(2):
        c = _ctx(s, g)
        runs.append(_update(c, s, g)[:3])
        c.close()
    for a, b in zip(*runs):
        assert np.array_equal(a, b)


@pytest.mark.parametrize("name", ["pend_ext_257", "skid_none_63"])
def test_device_drawn_noise(golden, name):
    """actions=None: the returned acts fed back to a fresh context reproduce costs and a_seq bit for bit; the same seed repeats the draws,
    another seed or the next tick does not; acts - a_seq0 has the law N(0, a_cov) (thresholds of
    test_particle_control_noise_inside_the_rollout_kernel: mean within 5 standard errors, spread within 6 %)"""
    s, g = cases.BY_TAG[name], golden("amppi_" + name)
    par, shared = _params(s, g), s["mode"] == "single"

    def tick(c, actions=None):
        return c.amppi_update(g["state"], actions, par, shared_params=shared, want_actions=True)

    c = _ctx(s, g, seed=7)
    c.set_a_seq(g["a_seq0"])
    costs, omega, a_seq, _, acts = tick(c)
    costs_n, _, _, _, acts_n = tick(c)  # the next tick: other draws
    assert not np.array_equal(acts, acts_n)
    fresh = _ctx(s, g, seed=99)
    fresh.set_a_seq(g["a_seq0"])
    costs_f, omega_f, a_seq_f, _, acts_f = tick(fresh, acts)
    assert np.array_equal(acts_f, acts) and np.array_equal(costs_f, costs) and np.array_equal(omega_f, omega) and np.array_equal(a_seq_f, a_seq)
    fresh.set_a_seq(g["a_seq0"])
    assert not np.array_equal(tick(fresh)[4], acts), "another seed draws other actions"
    again = _ctx(s, g, seed=7)
    again.set_a_seq(g["a_seq0"])
    assert np.array_equal(tick(again)[4], acts), "the same seed repeats the draws"
    # the law, on S = 4096 trajectories (32768 / 126976 draws per action dimension: the spread's sampling error is 0.4 % / 0.2 %)
    big = _ctx(s, g, seed=11, S=4096)
    big.set_a_seq(g["a_seq0"])
    acts_b = big.amppi_update(g["state"], None, None if par is None else np.resize(par, (4096, par.shape[1])), shared_params=shared, want_actions=True)[4]
    big.close()
    e = (acts_b.astype(np.float64) - g["a_seq0"].astype(np.float64)).reshape(-1, acts.shape[-1])
    cov = cases.a_cov_of(s).astype(np.float64)
    n = e.shape[0]
    for d in range(e.shape[1]):
        assert abs(e[:, d].mean()) < 5 * np.sqrt(cov[d, d] / n), (d, e[:, d].mean())
        assert abs(e[:, d].std() / np.sqrt(cov[d, d]) - 1.0) < 0.06, (d, e[:, d].std())
    if e.shape[1] == 2:
        rho = cov[0, 1] / np.sqrt(cov[0, 0] * cov[1, 1])
        assert abs(np.corrcoef(e.T)[0, 1] - rho) < 0.06
    for x in (c, fresh, again):
        x.close()


def test_one_update_is_one_launch(golden):
    s, g = cases.BY_TAG["pend_big_4099"], golden("amppi_pend_big_4099")
    c = _ctx(s, g)
    c.set_a_seq(g["a_seq0"])
    c.profile(True)
    c.amppi_update(g["state"], g["actions"], g["params"], want_states=True, want_actions=True)
    prof = c.profile_get()
    assert list(prof) == ["amppi_kernel"] and prof["amppi_kernel"][1] == 1, prof
    c.amppi_update(g["state"], None, g["params"], want_outputs=False)
    assert c.profile_get()["amppi_kernel"][1] == 2 and len(c.profile_get()) == 1
    c.close()


def test_deepcopy_gives_an_independent_controller(golden):
    s, g = cases.BY_TAG["cart_ut_64"], golden("amppi_cart_ut_64")
    model, inst, term = _mirror(s, g)
    model.params_dist = torch.distributions.MultivariateNormal(torch.tensor(g["dist_mean"]), covariance_matrix=torch.diag(torch.tensor(g["dist_std"]) ** 2))
    ctrl = _controller(s, g, model, inst, term)
    state, actions = torch.tensor(g["state"]), torch.tensor(g["actions"])
    before = copy.deepcopy(ctrl)  # (no context yet)
    ctrl.update_actions(model, state, actions)
    twin = copy.deepcopy(ctrl)
    assert twin._ctx is not ctrl._ctx and np.array_equal(twin.a_seq.numpy(), ctrl.a_seq.numpy())
    a1 = ctrl.a_seq.numpy().copy()
    twin.a_seq = torch.tensor(g["a_seq0"])
    assert np.array_equal(ctrl.a_seq.numpy(), a1), "the copy's sequence is its own"
    costs_t = twin.update_actions(model, state, actions)[0]
    costs_b = before.update_actions(model, state, actions)[0]
    assert _err(costs_t.numpy(), g, "costs") < float(g["tol_costs"]) and np.array_equal(costs_t.numpy(), costs_b.numpy())
    assert np.array_equal(ctrl.a_seq.numpy(), a1)


def test_refusals(golden):
    from dust_amd import Context, _lib as L
    from dust_amd.controllers import AMPPI
    from dust_amd.costs import QuadraticCost
    from dust_amd.models import CartPoleModel, Particle, PendulumModel

    s, g = cases.BY_TAG["pend_single_64"], golden("amppi_pend_single_64")
    kw = cases.context_kwargs(s)

    def status(fn):
        with pytest.raises(L.DustError) as e:
            fn()
        return e.value.status

    def refused(ckw, call, weights=None):
        """status of `call(context)` on a context of keywords ckw, which is closed again"""
        c = Context(**ckw)
        try:
            if weights is not None:
                c.set_param_weights(weights)
            return status(lambda: call(c))
        finally:
            c.close()

    single = lambda c: c.amppi_update(g["state"], None, g["params"], shared_params=True)
    assert refused(dict(kw, N=2), single) == L.ERR_INVALID  # n_policies != 1
    assert refused(dict(kw, S=65537, H=1), single) == L.ERR_UNSUPPORTED  # S > 65536
    assert status(lambda: Context(**dict(kw, H=129))) == L.ERR_UNSUPPORTED  # H da > 128
    # more than 4 uncertain parameters never reach the tick: dust_create refuses dim_p > 4 for every context
    assert status(lambda: Context(**dict(kw, uncertain_params=("g", "mass", "length", "a", "b")))) == L.ERR_INVALID
    assert refused(dict(kw, params_log_space=True), single) == L.ERR_UNSUPPORTED
    assert refused(dict(kw, uncertain_params=None, sampling=False),
                   lambda c: c.amppi_update(g["state"], None, np.ones((1, 1), np.float32), shared_params=True)) == L.ERR_INVALID  # rows, no parameters
    assert refused(kw, lambda c: c.amppi_roll(0)) == L.ERR_INVALID
    ps = cases.BY_TAG["part_none_64"]
    assert refused(cases.context_kwargs(ps, deterministic=False, noise_std=(0.1, 0.1)),
                   lambda c: c.amppi_update(np.zeros(4, np.float32))) == L.ERR_UNSUPPORTED  # control-channel noise
    assert refused(cases.context_kwargs(ps, control_type="velocity", target=(4.0, 4.5), w_state=(0.5, 0.5), w_term=(1.0, 1.0)),
                   lambda c: c.amppi_update(np.zeros(2, np.float32))) == L.ERR_UNSUPPORTED  # velocity control
    us, gu = cases.BY_TAG["pend_ut_65"], golden("amppi_pend_ut_65")
    assert refused(cases.context_kwargs(us), lambda c: c.amppi_update(g["state"]), weights=gu["loc_weights"]) == L.ERR_INVALID  # weights, no sigma points
    assert refused(cases.context_kwargs(us), lambda c: c.amppi_update(g["state"], None, gu["sigma_points"])) == L.ERR_INVALID  # n_params > 1, no weights

    # the class
    pend = PendulumModel(uncertain_params=("length",))
    from dust_amd.costs import PendulumQuadCos

    pc = PendulumQuadCos()
    with pytest.raises(ValueError, match="Invalid value for 'params_sampling'"):
        AMPPI(pend.observation_space, pend.action_space, 8, 64, inst_cost_fn=pc.inst_cost, term_cost_fn=pc.term_cost, params_sampling="all")
    with pytest.raises(ValueError, match="at least one cost function"):
        AMPPI(pend.observation_space, pend.action_space, 8, 64)
    state = torch.tensor([3.0, 0.0])
    cart = CartPoleModel()
    qc = QuadraticCost((0, 0, 0, 0), (1, 1, 1, 1), w_ctrl=(0.1,))
    with pytest.raises(NotImplementedError, match="w_ctrl"):
        AMPPI(cart.observation_space, cart.action_space, 8, 64, inst_cost_fn=qc.inst_cost, term_cost_fn=qc.term_cost,
              params_sampling="none").update_actions(cart, torch.zeros(4))
    noisy = Particle(**dict(cases.PART_ENV, deterministic=False), mass=2.0)
    with pytest.raises(NotImplementedError, match="deterministic"):
        AMPPI(noisy.observation_space, noisy.action_space, 8, 64, inst_cost_fn=noisy.default_inst_cost, term_cost_fn=noisy.default_term_cost,
              params_sampling="none").update_actions(noisy, torch.zeros(4))
    with pytest.raises(NotImplementedError):
        AMPPI(pend.observation_space, pend.action_space, 8, 64, inst_cost_fn=lambda x: x.sum(-1), term_cost_fn=pc.term_cost,
              params_sampling="none").update_actions(pend, state)

    class Other:
        family = "walker"

    with pytest.raises(NotImplementedError, match="no AMPPI kernel family"):
        AMPPI(pend.observation_space, pend.action_space, 8, 64, inst_cost_fn=pc.inst_cost, term_cost_fn=pc.term_cost).update_actions(Other(), state)
    with pytest.raises(NotImplementedError, match="128"):
        AMPPI(pend.observation_space, pend.action_space, 129, 64, inst_cost_fn=pc.inst_cost, term_cost_fn=pc.term_cost,
              params_sampling="none").update_actions(pend, state)
    with pytest.raises(NotImplementedError, match="65536"):
        AMPPI(pend.observation_space, pend.action_space, 8, 65537, inst_cost_fn=pc.inst_cost, term_cost_fn=pc.term_cost,
              params_sampling="none").update_actions(pend, state)
    many = CartPoleModel(uncertain_params=("g", "length", "mass_pole", "mass_cart", "f_mag"))
    q0 = QuadraticCost((0, 0, 0, 0), (1, 1, 1, 1))
    with pytest.raises(NotImplementedError, match="at most 4"):
        AMPPI(many.observation_space, many.action_space, 8, 64, inst_cost_fn=q0.inst_cost, term_cost_fn=q0.term_cost).update_actions(many, torch.zeros(4))
    from dust_amd.utils.utf import MerweScaledUTF

    ut = AMPPI(pend.observation_space, pend.action_space, 8, 64, inst_cost_fn=pc.inst_cost, term_cost_fn=pc.term_cost, params_sampling=MerweScaledUTF(n=1))

    class Mixture:  # the reference's third form (`.a`, `.xs[i].S`): a class it does not ship
        a, xs = None, None

    pend.params_dist = Mixture()
    with pytest.raises(NotImplementedError, match="covariance_matrix"):
        ut.update_actions(pend, state)
