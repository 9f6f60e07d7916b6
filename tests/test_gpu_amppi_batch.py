"""AMPPI over a batch of plants (dust_amppi_batch_* / Context.amppi_batch / dust_amd.controllers.BatchAMPPI): B independent ticks in one
launch.  A lone tick is pinned to the reference (tests/test_gpu_amppi.py); environment b of a batch is pinned to a lone tick on its
inputs BIT FOR BIT (np.array_equal) - the batched kernels run the lone kernel's body text on one environment's slices.  No tolerance
is introduced here; where a fixture rides in a batch, its own stored tolerances apply."""
import copy
import importlib.util
import os

import numpy as np
import pytest
import torch

import amppi_cases as cases
from helpers import elemerr

pytestmark = pytest.mark.gpu

B = 3
UP = dict(pendulum=("length",), particle=("mass",), skid=("x_icr", "wheel_radius", "axial_distance"), cartpole=("mass_pole", "length"))
FAMILIES = ("pendulum", "particle", "skid", "cartpole", "nav")  # nav: skid-steer with the navigation cost (amppi_skid_nav_batch_kernel)
MODES = ("none", "single", "extended", "ut")
SIZES = (1, 63, 257, 1021)  # one lane, a partial workgroup, two workgroups with a one-lane tail, four workgroups
NAV = dict(w_obs=10.0, cell_size=0.02)
QUANT = ("costs", "omega", "a_seq", "acts")
VARIANTS = ("costs_disco", "costs_noctrl", "costs_single", "costs_mean")


def _nav_map():
    """[80, 80] 0 / 1 occupancy in blocks of 2 cells (0.02 m cells: the trajectories of the skid-steer scenarios move a few centimetres
    and cross several blocks; seeded so that 55 - 70 % of their states lie on occupied cells)"""
    rng = np.random.default_rng(7)
    return np.ascontiguousarray(np.kron((rng.random((40, 40)) < 0.4).astype(np.float32), np.ones((2, 2), np.float32)))


def _scen(fam, mode, S, H=8, seed=900, **kw):
    family = "skid" if fam == "nav" else fam
    return dict(cases.A("batch_" + fam, family, S, H, mode, UP[family] if mode != "none" else (), seed, **kw), nav=fam == "nav")


def _tf(s):
    from dust_amd.utils.utf import MerweScaledUTF

    return MerweScaledUTF(n=len(s["up"]), alpha=cases.UT_ALPHA)


def _ctx(s, weights=None, **kw):
    from dust_amd import Context
    from oracle import grid_4x4_map

    grid = grid_4x4_map() if s["family"] == "particle" else (_nav_map() if s.get("nav") else None)
    c = Context(grid=grid, **cases.context_kwargs(s, **dict(NAV if s.get("nav") else {}, **kw)))
    if s["mode"] == "ut":
        c.set_param_weights(_tf(s).loc_weights.numpy() if weights is None else weights)
    return c


def _envs(s, n=B):
    """n environments of scenario s: amppi_cases.inputs on copies with other seeds (a_seq0, actions, parameter rows), shifted states,
    and in the sigma-point mode the points of a distribution whose mean moves with the environment"""
    ds = cases.FAMILY[s["family"]]["ds"]
    out = []
    for b in range(n):
        inp = cases.inputs(dict(s, seed=s["seed"] + 17 * b))
        inp["state"] = (inp["state"] + np.float32(0.05 * b) * np.arange(1, ds + 1, dtype=np.float32)).astype(np.float32)
        if s["mode"] == "ut":
            mean, std = cases.dist_of(s)
            mean = (mean * np.float32(1.0 + 0.03 * b)).astype(np.float32)
            inp["params"] = _tf(s).compute_sigma_points(torch.tensor(mean), torch.diag(torch.tensor(std) ** 2)).T.contiguous().numpy()
        out.append(inp)
    return out


def _stack(envs, k):
    return None if k not in envs[0] else np.stack([e[k] for e in envs])


def _lone(c, s, e, actions="given"):
    """one lone tick of context c on environment inputs e -> dict of QUANT"""
    c.set_a_seq(e["a_seq0"])
    costs, omega, a_seq, _, acts = c.amppi_update(e["state"], e["actions"] if actions == "given" else None, e.get("params"),
                                                  shared_params=s["mode"] == "single", want_actions=True)
    return dict(costs=costs, omega=omega, a_seq=a_seq, acts=acts)


def _batched(batch, s, envs, actions="given", active=None):
    costs, omega, a_seq, acts = batch.update(_stack(envs, "state"), _stack(envs, "actions") if actions == "given" else None, _stack(envs, "params"),
                                             shared_params=s["mode"] == "single", active=active, want_actions=True)
    return dict(costs=costs, omega=omega, a_seq=a_seq, acts=acts)


def _new_batch(s, envs, seeds=None, **kw):
    proto = _ctx(s, **kw)
    batch = proto.amppi_batch(len(envs), seeds)
    proto.close()  # (the batch keeps its own copy)
    batch.set_a_seq(_stack(envs, "a_seq0"))
    return batch


def _same(got, want, b, what=""):
    for q in QUANT:
        assert np.array_equal(got[q][b], want[q]), (what, b, q)


def _recorded(s):
    """scenario s on B environments from recorded inputs: every environment's costs, omega, updated sequence and stored actions are a
    lone tick's bits, and no two environments' outputs are equal (an environment that reads another's slice)"""
    envs = _envs(s)
    lone = _ctx(s)
    want = [_lone(lone, s, e) for e in envs]
    lone.close()
    batch = _new_batch(s, envs)
    got = _batched(batch, s, envs)
    assert np.array_equal(batch.get_a_seq(), got["a_seq"])
    batch.close()
    for b in range(B):
        _same(got, want[b], b, s["tag"])
    for q in QUANT:
        if q == "omega" and s["S"] == 1:
            continue  # (one trajectory takes the whole weight: omega = 0 in every environment)
        for b in range(B):
            for b2 in range(b + 1, B):
                assert not np.array_equal(got[q][b], got[q][b2]), (s["tag"], q, b, b2)


# ------------------------------------------------------------------------------------------------ 1. recorded inputs, bit for bit
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("fam", FAMILIES)
def test_recorded_inputs_bit_for_bit(fam, mode):
    for S in SIZES:
        _recorded(_scen(fam, mode, S))


@pytest.mark.parametrize("S", SIZES)
def test_full_action_covariance_and_clamp_bit_for_bit(S):
    """the 2 x 2 a_cov of skid_none_63 (the odd columns of the lambda term and of the drawn noise take their partner), and a start
    sequence ON the action bounds, where the final clamp acts"""
    _recorded(_scen("skid", "none", S, a_cov=cases.BY_TAG["skid_none_63"]["a_cov"]))
    _recorded(_scen("pendulum", "extended", S, a_seq0="edge"))


def test_the_navigation_cost_is_in_the_batch():
    """the obstacle term moves the costs of the `nav` family (otherwise its cases would repeat the plain skid-steer ones)"""
    s = _scen("nav", "none", 63)
    envs = _envs(s)
    nav, plain = _new_batch(s, envs), _new_batch(dict(s, nav=False), envs)
    a, b = _batched(nav, s, envs)["costs"], _batched(plain, s, envs)["costs"]
    nav.close(); plain.close()
    assert np.abs(a - b).max() >= NAV["w_obs"] * 0.5 and not np.array_equal(a, b)


# ------------------------------------------------------------------------------------------------ 2. a fixture in the middle slot
def _err(got, g, q):
    return min(elemerr(got, g[q]), elemerr(got, cases.twin(g, q)))


@pytest.mark.parametrize("name", cases.CLASS_CASES)
def test_fixture_in_the_middle_slot(golden, name):
    """slot 1 of 3 holds a fixture's inputs, slots 0 and 2 shifted states: slot 1 meets the fixture's stored tolerances and stays outside
    them for every power variant the fixture carries (as test_fixture_through_the_context)"""
    s, g = cases.BY_TAG[name], golden("amppi_" + name)
    fix = dict(state=g["state"], a_seq0=g["a_seq0"], actions=g["actions"])
    par = g["sigma_points"] if s["mode"] == "ut" else g.get("params")
    if par is not None:
        fix["params"] = par
    envs = [dict(fix, state=(g["state"] + np.float32(d)).astype(np.float32)) for d in (-0.1, 0.0, 0.1)]
    batch = _new_batch(s, envs, weights=g["loc_weights"] if s["mode"] == "ut" else None)
    got = _batched(batch, s, envs)
    batch.close()
    errs = dict(costs=_err(got["costs"][1], g, "costs"), omega=_err(got["omega"][1], g, "omega"), a_seq1=_err(got["a_seq"][1], g, "a_seq1"))
    print(name, " ".join("%s %.2e / %.1e" % (q, e, float(g["tol_" + q])) for q, e in errs.items()))
    for q, e in errs.items():
        assert e < float(g["tol_" + q]), (q, e, float(g["tol_" + q]))
    assert np.array_equal(got["acts"][1], g["actions"])
    for v in VARIANTS:
        if v in g:
            assert elemerr(got["costs"][1], g[v]) > float(g["tol_costs"]), v
    if "a_seq1_noclamp" in g:
        assert elemerr(got["a_seq"][1], g["a_seq1_noclamp"]) > float(g["tol_a_seq1"])
    for b in (0, 2):
        assert not np.array_equal(got["costs"][b], got["costs"][1])


# ------------------------------------------------------------------------------------------------ 3. device-drawn noise
def test_device_drawn_noise_continues_each_seeds_stream():
    """seeds (7, 7, 9), equal inputs, three ticks: environments 0 and 1 agree bit for bit on every tick, environment 2 differs, each is a
    lone context of its seed making the same three calls - and a tick's returned actions fed back as recorded actions repeat its bits"""
    s = _scen("skid", "extended", 257, a_cov=cases.BY_TAG["skid_none_63"]["a_cov"])
    e = _envs(s, 1)[0]
    envs, seeds = [e] * 3, (7, 7, 9)
    batch = _new_batch(s, envs, seeds)
    lone = {sd: _ctx(s, seed=sd) for sd in set(seeds)}
    for c in lone.values():
        c.set_a_seq(e["a_seq0"])
    start = _stack(envs, "a_seq0")
    for tick in range(3):
        got = _batched(batch, s, envs, actions="drawn")
        want = {}
        for sd, c in lone.items():
            costs, omega, a_seq, _, acts = c.amppi_update(e["state"], None, e["params"], want_actions=True)
            want[sd] = dict(costs=costs, omega=omega, a_seq=a_seq, acts=acts)
        for b, sd in enumerate(seeds):
            _same(got, want[sd], b, "tick %d" % tick)
        for q in QUANT:
            assert np.array_equal(got[q][0], got[q][1]) and not np.array_equal(got[q][0], got[q][2]), (tick, q)
        again = _new_batch(s, envs, (1, 2, 3))
        again.set_a_seq(start)
        fed = again.update(_stack(envs, "state"), got["acts"], _stack(envs, "params"), want_actions=True)
        again.close()
        for q, v in zip(QUANT, fed):
            assert np.array_equal(v, got[q]), (tick, q)
        start = got["a_seq"]
    batch.close()
    for c in lone.values():
        c.close()


# ------------------------------------------------------------------------------------------------ 4. the active mask
def test_active_mask():
    """three ticks with rolls under masks (1,1,1), (1,0,1), (1,1,0), device-drawn noise: each environment equals a lone context that made
    only its active calls; an inactive environment's a_seq is unchanged and its rows of the outputs stay as the caller filled them"""
    s = _scen("pendulum", "extended", 257)
    envs, seeds = _envs(s), (3, 4, 5)
    batch = _new_batch(s, envs, seeds)
    lone = [_ctx(s, seed=sd) for sd in seeds]
    for c, e in zip(lone, envs):
        c.set_a_seq(e["a_seq0"])
    for mask in ((1, 1, 1), (1, 0, 1), (1, 1, 0)):
        before = batch.get_a_seq()
        got = _batched(batch, s, envs, actions="drawn", active=mask)  # (the wrapper pre-fills every output with NaN)
        after = batch.get_a_seq()
        for b, (c, e) in enumerate(zip(lone, envs)):
            if mask[b]:
                costs, omega, a_seq, _, acts = c.amppi_update(e["state"], None, e["params"], want_actions=True)
                _same(got, dict(costs=costs, omega=omega, a_seq=a_seq, acts=acts), b, str(mask))
                assert np.array_equal(after[b], a_seq)
                c.amppi_roll(1)
            else:
                assert np.array_equal(after[b], before[b]), "an inactive environment's sequence moved"
                for q in QUANT:
                    assert np.isnan(got[q][b]).all(), (mask, b, q)
        batch.roll(1, active=mask)
        rolled = batch.get_a_seq()
        for b, c in enumerate(lone):
            assert np.array_equal(rolled[b], c.get_a_seq()), (mask, b)
    batch.close()
    for c in lone:
        c.close()


# ------------------------------------------------------------------------------------------------ 5. one launch
def test_one_tick_is_one_launch():
    s = _scen("pendulum", "extended", 257)
    envs = _envs(s, 5)
    batch = _new_batch(s, envs)
    batch.ctx.profile(True)
    _batched(batch, s, envs)
    prof = batch.ctx.profile_get()
    assert list(prof) == ["amppi_kernel"] and prof["amppi_kernel"][1] == 1, prof
    batch.update(_stack(envs, "state"), None, _stack(envs, "params"), active=(1, 0, 1, 1, 0), want_outputs=False)
    prof = batch.ctx.profile_get()
    assert list(prof) == ["amppi_kernel"] and prof["amppi_kernel"][1] == 2, prof
    batch.roll(1)
    prof = batch.ctx.profile_get()
    assert prof["amppi_kernel"][1] == 2 and prof["forward(finalize+roll)"][1] == 1 and len(prof) == 2, prof
    batch.close()


# ------------------------------------------------------------------------------------------------ 6. repeatability
def test_a_cloned_batch_repeats_the_bits():
    """B = 4, S = 1021 (four workgroups per environment; whichever arrives last reduces): the same call on a cloned batch gives the same
    bits, from recorded actions and from device-drawn ones"""
    s = _scen("pendulum", "extended", 1021)
    envs = _envs(s, 4)
    batch = _new_batch(s, envs, (1, 2, 3, 4))
    for actions in ("given", "drawn"):
        twin = batch.clone()
        a, b = _batched(batch, s, envs, actions), _batched(twin, s, envs, actions)
        twin.close()
        for q in QUANT:
            assert np.array_equal(a[q], b[q]), (actions, q)
    batch.close()


# ------------------------------------------------------------------------------------------------ 7. deep copy mid-loop
def test_deep_copy_mid_loop():
    s = _scen("cartpole", "ut", 63)
    envs = _envs(s)
    batch = _new_batch(s, envs, (11, 12, 13))
    _batched(batch, s, envs, "drawn")
    batch.roll(1)
    twin = copy.deepcopy(batch)
    assert twin is not batch and np.array_equal(twin.get_a_seq(), batch.get_a_seq()) and np.array_equal(twin.get_actions(), batch.get_actions())
    kept = twin.get_a_seq()
    a1 = _batched(batch, s, envs, "drawn")  # advancing the original ...
    assert np.array_equal(twin.get_a_seq(), kept) and not np.array_equal(batch.get_a_seq(), kept)  # ... does not move the copy
    b1 = _batched(twin, s, envs, "drawn")  # the copy draws what the original drew: same stream position, same sequence
    batch.roll(2); twin.roll(2)
    a2, b2 = _batched(batch, s, envs, "drawn"), _batched(twin, s, envs, "drawn")
    batch.close(); twin.close()
    for a, b in ((a1, b1), (a2, b2)):
        for q in QUANT:
            assert np.array_equal(a[q], b[q]), q
    assert not np.array_equal(a1["acts"], a2["acts"])


# ------------------------------------------------------------------------------------------------ 8. refusals, before any launch
def test_refusals(golden):
    from dust_amd import Context, _lib as L

    s = _scen("pendulum", "single", 64)
    envs = _envs(s)
    kw = cases.context_kwargs(s)
    states, rows = _stack(envs, "state"), _stack(envs, "params")

    def refused(fn, status, match):
        with pytest.raises(L.DustError, match=match) as e:
            fn()
        assert e.value.status == status, (e.value.status, status, str(e.value))

    def create(ckw, n=B, grid=None, weights=None):
        c = Context(grid=grid, **ckw)
        try:
            if weights is not None:
                c.set_param_weights(weights)
            return c.amppi_batch(n)
        finally:
            c.close()

    refused(lambda: create(dict(kw, N=2)), L.ERR_INVALID, r"n_policies = 1 \(got 2\)")
    refused(lambda: create(kw, 0), L.ERR_INVALID, r"n_env = 0 outside \[1, 65535\]")
    refused(lambda: create(kw, 65536), L.ERR_INVALID, r"n_env = 65536 outside \[1, 65535\]")
    refused(lambda: create(dict(kw, params_log_space=True)), L.ERR_UNSUPPORTED, "params_log_space")
    ps = cases.BY_TAG["part_none_64"]
    from oracle import grid_4x4_map

    refused(lambda: create(cases.context_kwargs(ps, deterministic=False, noise_std=(0.1, 0.1)), grid=grid_4x4_map()), L.ERR_UNSUPPORTED,
            "acceleration control and no control-channel noise")
    refused(lambda: create(cases.context_kwargs(ps, control_type="velocity", target=(4.0, 4.5), w_state=(0.5, 0.5), w_term=(1.0, 1.0)), grid=grid_4x4_map()),
            L.ERR_UNSUPPORTED, "acceleration control and no control-channel noise")

    batch = create(kw)
    batch.ctx.profile(True)
    single = dict(params=rows, shared_params=True)
    refused(lambda: batch.update(states, flags=L.STORE_STATES, **single), L.ERR_UNSUPPORTED, "DUST_STORE_STATES")
    refused(lambda: batch.update(states, flags=L.EPS_F16, **single), L.ERR_UNSUPPORTED, "binary16")
    refused(lambda: batch.update(states, flags=L.STORE_F16, **single), L.ERR_UNSUPPORTED, "binary16")
    refused(lambda: batch.update(None, **single), L.ERR_INVALID, "null argument")
    refused(lambda: batch.roll(0), L.ERR_INVALID, r"steps >= 1")
    refused(lambda: batch.get_actions(), L.ERR_STATE, "no batched tick has run yet")
    assert batch.ctx.profile_get() == {}, "a refused call launched something"
    batch.close()

    plain = create(dict(kw, uncertain_params=None, sampling=False))
    plain.ctx.profile(True)
    refused(lambda: plain.update(states, params=np.ones((B, 1, 1), np.float32), shared_params=True), L.ERR_INVALID, r"dim_p = 0")
    assert plain.ctx.profile_get() == {}
    plain.close()

    us, gu = cases.BY_TAG["pend_ut_65"], golden("amppi_pend_ut_65")
    ut = create(cases.context_kwargs(us), weights=gu["loc_weights"])
    ut.ctx.profile(True)
    refused(lambda: ut.update(states), L.ERR_INVALID, "sigma-point weights are set")
    assert ut.ctx.profile_get() == {}
    ut.close()


# ------------------------------------------------------------------------------------------------ 9. the class
def _mirror(s):
    """the repo's own model and cost classes for scenario s -> (model, inst_cost_fn, term_cost_fn)"""
    from dust_amd.costs import PendulumQuadCos, QuadraticCost
    from dust_amd.models import PendulumModel, SkidSteerRobot

    f = cases.FAMILY[s["family"]]
    up = tuple(s["up"]) or None
    if s["family"] == "pendulum":
        cost = PendulumQuadCos(f["w_cos"], f["w_vel"])
        return PendulumModel(uncertain_params=up, **f["defaults"]), cost.inst_cost, cost.term_cost
    cost = QuadraticCost(f["goal"], f["w_state"], f["w_term"])
    m = SkidSteerRobot(f["dt"], min_wheel_speed=torch.tensor(f["lo"]), max_wheel_speed=torch.tensor(f["hi"]), uncertain_params=up, **f["defaults"])
    return m, cost.inst_cost, cost.term_cost


def _ctor_args(s, model, inst, term, a_seq0):
    f = cases.FAMILY[s["family"]]
    return (model.observation_space, model.action_space, s["H"], s["S"]), dict(
        lambda_=f["lam"], a_cov=torch.tensor(cases.a_cov_of(s)), inst_cost_fn=inst, term_cost_fn=term, params_sampling=s["mode"],
        init_actions=torch.tensor(a_seq0))


def _feed(model, rows):
    """model.sample_params hands out the recorded rows, one set per call, in the order of the list"""
    queue = [np.asarray(r) for r in rows]
    model.sample_params = lambda n: model.params_to_dict(torch.as_tensor(queue.pop(0))[:n])
    return queue


@pytest.mark.parametrize("name", ["pend_ext_257", "skid_none_63"])
def test_class_equals_b_controllers(golden, name):
    """BatchAMPPI with explicit actions and params against B AMPPI objects, bit for bit; then the class's own draws - once per ACTIVE
    environment, in environment order"""
    from dust_amd.controllers import AMPPI, BatchAMPPI

    s = cases.BY_TAG[name]
    envs = _envs(s)
    model, inst, term = _mirror(s)
    args, kw = _ctor_args(s, model, inst, term, envs[0]["a_seq0"])
    want = []
    for e in envs:
        ctrl = AMPPI(*args, **kw)
        ctrl.a_seq = torch.tensor(e["a_seq0"])
        if "params" in e:
            _feed(model, [e["params"]])
        costs, _, acts, omega = ctrl.update_actions(model, torch.tensor(e["state"]), torch.tensor(e["actions"]))
        want.append(dict(costs=costs.numpy(), omega=omega.numpy(), a_seq=ctrl.a_seq.numpy(), acts=acts.numpy()))
    bc = BatchAMPPI(B, *args, **kw)
    assert tuple(bc.a_seq.shape) == (B, s["H"], cases.FAMILY[s["family"]]["da"])
    bc.a_seq = torch.tensor(_stack(envs, "a_seq0"))
    par = _stack(envs, "params")
    costs, states, acts, omega = bc.update_actions(model, torch.tensor(_stack(envs, "state")), torch.tensor(_stack(envs, "actions")),
                                                   params=None if par is None else torch.tensor(par))
    assert states is None
    got = dict(costs=costs.numpy(), omega=omega.numpy(), a_seq=bc.a_seq.numpy(), acts=acts.numpy())
    for b in range(B):
        _same(got, want[b], b, name)
    if par is not None:  # the class's own draws under a mask: two calls of sample_params, for environments 0 and 2
        bc.a_seq = torch.tensor(_stack(envs, "a_seq0"))
        left = _feed(model, [envs[0]["params"], envs[2]["params"], envs[1]["params"]])
        bc.return_rollouts = False
        costs, _, acts, omega = bc.update_actions(model, torch.tensor(_stack(envs, "state")), torch.tensor(_stack(envs, "actions")), active=(1, 0, 1))
        assert acts is None and len(left) == 1
        for b in (0, 2):
            assert np.array_equal(costs.numpy()[b], want[b]["costs"]) and np.array_equal(bc.a_seq.numpy()[b], want[b]["a_seq"])
        assert np.isnan(costs.numpy()[1]).all() and np.isnan(omega.numpy()[1]).all() and np.array_equal(bc.a_seq.numpy()[1], envs[1]["a_seq0"])
    twin = copy.deepcopy(bc)
    assert twin._batch is not bc._batch and np.array_equal(twin.a_seq.numpy(), bc.a_seq.numpy())


def test_closed_loop_through_the_class(golden):
    """pend_loop in the middle slot of three: update_actions from recorded actions and rows, the plants' steps with the first planned
    actions, roll(1) - four ticks, slot 1 at the fixture's own tolerances, as test_gpu_amppi.py's closed loop"""
    from dust_amd.controllers import BatchAMPPI
    from dust_amd.models import PendulumModel

    s, g = cases.LOOP, golden("amppi_pend_loop")
    model, inst, term = _mirror(s)
    plant = PendulumModel()
    args, kw = _ctor_args(s, model, inst, term, g["a_seq0"])
    bc = BatchAMPPI(B, *args, **kw)
    bc.return_rollouts = False
    states = torch.tensor(np.stack([g["state"] + np.float32(d) for d in (-0.2, 0.0, 0.2)]))
    for k in range(s["ticks"]):
        _feed(model, [g["params"][k]] * B)
        costs, _, _, omega = bc.update_actions(model, states, torch.tensor(np.stack([g["actions"][k]] * B)))
        a_seq = bc.a_seq
        states = plant.step(states, a_seq[:, 0])
        got = dict(costs=costs.numpy()[1], omega=omega.numpy()[1], a_seq1=a_seq.numpy()[1], plant=states.numpy()[1])
        for q, v in got.items():
            e = min(elemerr(v, g[q][k]), elemerr(v, g[q + "_f64"][k]))
            assert e < float(g["tol_" + q][k]), (k, q, e)
        for v in ("costs_disco", "costs_noctrl", "costs_single"):
            assert elemerr(got["costs"], g[v][k]) > float(g["tol_costs"][k]), (k, v)
        assert not np.array_equal(costs.numpy()[0], costs.numpy()[1]) and not np.array_equal(costs.numpy()[2], costs.numpy()[1])
        bc.roll(1)
        rolled = bc.a_seq.numpy()
        assert np.array_equal(rolled[:, :-1], a_seq.numpy()[:, 1:]) and not rolled[:, -1].any()
    bc.roll(s["H"] + 3, active=(1, 0, 1))
    assert not bc.a_seq.numpy()[[0, 2]].any() and np.array_equal(bc.a_seq.numpy()[1], rolled[1])


def test_example_runs_three_periods():
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples", "amppi_batch_example.py")
    spec = importlib.util.spec_from_file_location("amppi_batch_example", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    avg = mod.run(n_envs=4, steps=3, horizon=8, n_samples=64, quiet=True)
    assert tuple(avg.shape) == (4,) and bool(torch.isfinite(avg).all()) and len(set(avg.tolist())) == 4
