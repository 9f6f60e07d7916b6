"""MultiDISCO over a batch of plants on the device (csrc/disco_batch.hpp disco_batch_kernel / disco_skid_nav_batch_kernel,
dust_disco_batch_forward / _step / _tick, `DiscoBatch`, `BatchDISCO`).  Every np.array_equal below is bit for bit.

1. invariance: an environment computes the same alone, in slots 0 / 2 / 4 of five, beside inactive neighbours (whose rows and state stay
   untouched) and from a clone taken mid-loop;
2. tick is forward then step, on every getter and next_actions, with recorded and with device noise;
3. stage-wise against the float64 restatement of tests/disco_cases.py, fed the device's own actions and costs: omega, a_mat, a_mix,
   next_actions, a_seq and the rolled rows within tolerances measured from the restatement alone; the costs themselves against the
   float64 rollouts (the families whose instantaneous cost has no action term), and every restated wrong form kept away;
4. against a lone context over three ticks in first-divergence form, at the tolerances of tests/test_gpu_svmpc_batch.py (costs 2e-5
   element-wise, what lies downstream of exp(-cost / temp) 5e-4); device-drawn actions bit-equal to the lone context's;
5. the reference: the closed-loop fixtures tests/golden/disco_loop_*.npz (four periods of its own forward, step and plant per case) and the
   existing disco_mppi / disco_ut fixtures in the middle slot of three, at the tolerances stored in the former and at
   test_gpu_parity.py's and test_gpu_mirror_api.py's for the latter;
6. one launch per call, every refusal with zero launches and unchanged getters;
7. `BatchDISCO` against B `MultiDISCO` objects with a deep copy mid-loop.
"""
import copy
import functools

import numpy as np
import pytest
import torch

import disco_cases as dc
from disco_helpers import COST_TOL, EXP_TOL, GETTERS, _L, _batch, _pair, _proto, _records, _same, _sub
from helpers import elemerr, relerr

pytestmark = pytest.mark.gpu

def _tick(b, case, inp, envs, recorded, active=None):
    """one tick of the case on these environments -> next_actions"""
    return b.tick(_sub(inp, envs, "states"), case["strategy"], case["steps"], actions=_sub(inp, envs, "actions") if recorded else None,
                  params=_sub(inp, envs, "params"), ext_actions=_sub(inp, envs, "ext"), active=active, around_a_mat=recorded)


# ------------------------------------------------------------------------------------------------ 1. invariance
@pytest.mark.parametrize("cid", ["mppi", "disco", "multi_arg", "wave63", "part", "skid_nav_sigma"])
def test_an_environment_does_not_depend_on_its_batch(cid):
    case = dc.BY_ID[cid]
    inp, e, B = dc.inputs(case), 1, case["B"]

    def run(envs, active=None, clone_after=None):
        """two ticks (recorded noise, then device noise) -> ([(next, records)] per tick, the same from a clone taken after `clone_after`)"""
        b, twin, out, tout = _batch(case, inp, envs), None, [], []
        for t, rec in enumerate((True, False)):
            out.append((_tick(b, case, inp, envs, rec, active), _records(b)))
            if twin is not None:
                tout.append((_tick(twin, case, inp, envs, rec, active), _records(twin)))
            if clone_after == t:
                twin = b.clone()
        b.close()
        if twin is not None:
            twin.close()
        return out, tout

    alone, _ = run([e])
    assert not np.array_equal(alone[0][1]["A_MAT"], alone[1][1]["A_MAT"])
    envs = [e, 0, e, (e + 1) % B, e]  # slots 0 / 2 / 4 of five, and a clone after the first tick
    five, twin = run(envs, clone_after=0)
    for t in range(2):
        for slot in (0, 2, 4):
            assert np.array_equal(five[t][0][slot], alone[t][0][0]), (t, slot)
            for k in GETTERS:
                assert np.array_equal(five[t][1][k][slot], alone[t][1][k][0]), (t, slot, k)
    assert np.array_equal(twin[0][0], five[1][0])
    _same(twin[0][1], five[1][1])
    # beside inactive neighbours: a tick of everybody first, so that the neighbours have rows to keep
    envs = [0, e, 0]
    three, lone = _batch(case, inp, envs), _batch(case, inp, [e])
    _tick(three, case, inp, envs, True)
    _tick(lone, case, inp, [e], True)
    before = _records(three)
    nxt = _tick(three, case, inp, envs, False, active=[0, 1, 0])
    solo = _tick(lone, case, inp, [e], False)
    got, want = _records(three), _records(lone)
    three.close()
    lone.close()
    assert np.array_equal(nxt[1], solo[0]) and np.isnan(nxt[[0, 2]]).all()
    for k in GETTERS:
        assert np.array_equal(got[k][1], want[k][0]), k
        assert np.array_equal(got[k][[0, 2]], before[k][[0, 2]]), k


# ------------------------------------------------------------------------------------------------ 2. tick = forward, then step
@pytest.mark.parametrize("recorded", [True, False], ids=["recorded", "device"])
@pytest.mark.parametrize("cid", dc.IDS)
def test_tick_is_forward_then_step(cid, recorded):
    case = dc.BY_ID[cid]
    inp, envs = dc.inputs(case), range(case["B"])
    one, two = _batch(case, inp), _batch(case, inp)
    for _ in range(2):  # (the second round starts from rolled rows and a moved noise position)
        nxt = _tick(one, case, inp, envs, recorded)
        two.forward(inp["states"], inp["actions"] if recorded else None, inp["params"], around_a_mat=recorded)
        nxt2 = two.step(case["strategy"], case["steps"], inp["ext"])
        assert np.array_equal(nxt, nxt2) and np.isfinite(nxt).all() and nxt.shape == (case["B"], case["steps"], dc.family(case)["da"])
        _same(_records(one), _records(two))
    one.close()
    two.close()


# ------------------------------------------------------------------------------------------------ 3. stage-wise against float64
@functools.lru_cache(maxsize=None)
def _staged(cid, recorded):
    """forward (actions kept), the getters, then step and the getters again, per environment"""
    L = _L()
    case = dc.BY_ID[cid]
    inp = dc.inputs(case)
    b = _batch(case, inp)
    b.forward(inp["states"], inp["actions"] if recorded else None, inp["params"], keep_actions=True)  # recorded: eps = a - a_seq
    fw = _records(b, actions=True)
    nxt = b.step(case["strategy"], case["steps"], inp["ext"])
    st = _records(b)
    b.close()
    return inp, fw, nxt, st


@pytest.mark.parametrize("recorded", [True, False], ids=["recorded", "device"])
@pytest.mark.parametrize("cid", dc.IDS)
def test_stages_against_float64(cid, recorded):
    case = dc.BY_ID[cid]
    inp, fw, nxt, st = _staged(cid, recorded)
    tol = dc.stage_tolerance(case)
    if recorded:
        assert np.array_equal(fw["ACTIONS"], inp["actions"])
    worst = {}
    for b in range(case["B"]):
        ref = dc.stages(case, inp["a_mat"][b], inp["a_seq"][b], fw["ACTIONS"][b], fw["COSTS"][b], not recorded, inp["ext"][b])
        got = dict(omega=fw["OMEGA"][b], a_mat1=fw["A_MAT"][b], a_mix=fw["A_MIX"][b], next=nxt[b], a_seq=st["A_SEQ"][b], a_mat=st["A_MAT"][b])
        for k in dc.STAGES:
            worst[k] = max(worst.get(k, 0.0), elemerr(got[k], ref[k]) / tol[k])
        assert abs(float(fw["OMEGA"][b].sum(0).max()) - 1.0) < 1e-5 and abs(float(fw["A_MIX"][b].sum()) - 1.0) < 1e-5
        # the rolled rows: zeros behind, exactly
        sh = case["steps"]
        assert not st["A_SEQ"][b][case["H"] - sh:].any() and not st["A_MAT"][b][:, case["H"] - sh:].any()
    print("%-15s %-8s " % (cid, "recorded" if recorded else "device") + "  ".join("%s %.2f" % (k, worst[k]) for k in dc.STAGES) + "  (tolerances)")
    for k in dc.STAGES:
        assert worst[k] < 1.0, (cid, k, worst[k], tol[k])
    if case["tie"] and recorded:  # identical rows, identical recorded actions - an exact tie of a_mix: argmax is index 0, whose clamped row went out
        assert np.array_equal(fw["A_MIX"][:, 0], fw["A_MIX"][:, 1])
        lo, hi = (np.asarray(dc.family(case)[k], np.float32) for k in ("lo", "hi"))
        assert np.array_equal(nxt[:, 0], np.clip(fw["A_MAT"][:, 0, 0], lo, hi))


@pytest.mark.parametrize("cid", [c for c in dc.IDS if dc.BY_ID[c]["family"] != "particle" and not dc.BY_ID[c]["nav"] and c != "corner"])
def test_costs_against_float64_rollouts(cid):
    """the COSTS record against the restated rollouts and control cost in float64, on the recorded actions, within the tolerance
    tests/disco_cases.py measures from the restatement alone; every wrong form the restatement has stays at least 5 tolerances away.
    (Particle's cost has an action term and the navigation term its own restatement, tests/skid_nav_cases.py: both are held through the
    lone context, item 4.)"""
    case = dc.BY_ID[cid]
    inp, fw, _, _ = _staged(cid, True)
    tol = dc.cost_tolerance(case)
    for b in range(case["B"]):
        ref = dc.final_costs(case, inp, b)
        err = elemerr(fw["COSTS"][b], ref)
        far = {}
        if case["ctrl_penalty"] != 1.0:
            far["noctrl"] = elemerr(dc.final_costs(case, inp, b, variant="noctrl"), ref) / tol
        if case["sigma"]:
            far["uniform"] = elemerr(dc.final_costs(case, inp, b, uniform_weights=True), ref) / tol
        print("%-15s env %d costs err %.2e tol %.2e  " % (cid, b, err, tol) + "  ".join("%s %.0f" % kv for kv in sorted(far.items())))
        assert err < tol, (cid, b, err, tol)
        for k, v in far.items():
            assert v >= 5.0, (cid, k, v)


# ------------------------------------------------------------------------------------------------ 4. a lone context
@pytest.mark.parametrize("cid", ["mppi", "disco", "multi_avg", "multi_arg", "wave257", "part", "skid", "skid_nav_sigma", "cart"])
def test_batch_equals_a_lone_context(cid):
    """Three ticks of a lone context and of environment 1 of a batch of two, side by side, on device-drawn noise; after every tick the
    lone context takes over the batch's a_mat and a_seq, so every tick is a first-divergence comparison"""
    L = _L()
    case = dc.BY_ID[cid]
    inp = dc.inputs(case, 2)
    lone = _proto(case)
    lone.set_a_mat(inp["a_mat"][1])
    lone.set_a_seq(inp["a_seq"][1])
    batch = lone.disco_batch(2, seeds=[5, case["seed"]])  # environment 1 draws with the lone context's key
    batch.set(L.DCB_A_MAT, inp["a_mat"])
    batch.set(L.DCB_A_SEQ, inp["a_seq"])
    st, strat, steps = inp["states"], case["strategy"], case["steps"]
    for t in range(3):
        params = None if inp["params"] is None else (inp["params"] * np.float32(1.0 + 0.01 * t)).astype(np.float32)
        costs, _, acts, omega = lone.disco_forward(st[1], None, None if params is None else params[1], want_actions=True)
        batch.forward(st, None, params, keep_actions=True)
        got = _records(batch, actions=True)
        assert np.array_equal(got["ACTIONS"][1], acts), t  # the lone context's draws, bit for bit
        assert not np.array_equal(got["ACTIONS"][0], acts)
        errs = dict(costs=(elemerr(got["COSTS"][1], costs), COST_TOL), omega=(elemerr(got["OMEGA"][1], omega), EXP_TOL),
                    a_mat1=(elemerr(got["A_MAT"][1], lone.get_a_mat()), EXP_TOL))
        nl = lone.disco_step(strat, steps, inp["ext"][1] if strat == "external" else None)
        nb = batch.step(strat, steps, inp["ext"] if strat == "external" else None)
        got = _records(batch)
        errs.update(a_mix=(elemerr(got["A_MIX"][1], lone.get_a_mix()), EXP_TOL), next=(elemerr(nb[1], nl), EXP_TOL),
                    a_seq=(elemerr(got["A_SEQ"][1], lone.get_a_seq()), EXP_TOL), a_mat=(elemerr(got["A_MAT"][1], lone.get_a_mat()), EXP_TOL))
        print("%-15s tick %d  " % (cid, t) + "  ".join("%s %.1e" % (k, v[0]) for k, v in errs.items()))
        for k, (err, tol) in errs.items():
            assert err < tol, (cid, t, k, err, tol)
        lone.set_a_mat(got["A_MAT"][1])
        lone.set_a_seq(got["A_SEQ"][1])
    batch.close()
    lone.close()


# ------------------------------------------------------------------------------------------------ 5. the reference's fixtures
def test_disco_mppi_fixture_in_the_middle_slot(golden):
    """tests/test_gpu_parity.py test_disco_mppi's stages and tolerances, through the batch"""
    from dust_amd import Context

    L = _L()
    g = golden("disco_mppi")
    N, H, S = int(g["N"]), int(g["H"]), int(g["S"])
    temp, a_reg = float(g["temperature"]), float(g["a_reg"])
    c = Context(model="pendulum", N=N, S=S, M=1, H=H, temperature=temp, ctrl_penalty=1.0 - a_reg / temp, sigma_a=float(g["sigma_a"]), alpha=1.0 / temp)
    b = c.disco_batch(3)
    c.close()
    rng = np.random.default_rng(3)
    a_mat = np.stack([g["a_mat0"] + 0.1 * rng.standard_normal(g["a_mat0"].shape).astype(np.float32), g["a_mat0"], 0.5 * g["a_mat0"]])
    acts = np.stack([g["actions"][0][::-1], g["actions"][0], g["actions"][0] + np.float32(0.1)])
    states = np.stack([g["state"] + np.float32(0.1), g["state"], g["state"] - np.float32(0.2)])
    b.set(L.DCB_A_MAT, a_mat)
    b.forward(states, acts, around_a_mat=True)
    got = _records(b)
    TOL = 2e-5
    assert elemerr(got["COSTS"][1], g["costs"]) < TOL
    assert relerr(got["OMEGA"][1], g["omega"]) < 2e-4
    assert relerr(got["A_MAT"][1], g["a_mat1"]) < 1e-4
    assert relerr(got["A_MIX"][1], g["a_mix"]) < 2e-4
    assert elemerr(got["COSTS"][0], g["costs"]) > 100 * TOL  # (the neighbours are other problems)
    for strat in ("argmax", "average"):
        cc = b.clone()
        nxt = cc.step(strat, 2)
        assert relerr(nxt[1], g["step_%s_actions" % strat]) < 1e-4
        assert relerr(cc.get(L.DCB_A_SEQ)[1], g["step_%s_a_seq" % strat]) < 1e-4
        assert relerr(cc.get(L.DCB_A_MAT)[1], g["step_%s_a_mat" % strat]) < 1e-4
        cc.close()
    ext = np.stack([g["step_external_in"]] * 3)
    nxt = b.step("external", 1, ext)
    assert np.array_equal(nxt[1], g["step_external_actions"])
    assert np.array_equal(b.get(L.DCB_A_SEQ)[1], g["step_external_a_seq"])
    b.close()


@pytest.mark.parametrize("cid", dc.LOOP_IDS)
def test_reference_loop_fixture_in_the_middle_slot(golden, cid):
    """tests/golden/disco_loop_<case>.npz: four closed-loop periods of the reference's own MultiDISCO.forward (its draws recorded), step and
    plant.  The middle environment of three is fed the reference's recorded state and actions every period and carries its own a_mat and
    a_seq from period to period; every quantity within the tolerance stored in the fixture (of the fp32 run or of its float64 twin)"""
    L = _L()
    case, g = dc.BY_ID[cid], golden("disco_loop_" + cid)
    T = int(g["T"])
    c = _proto(case)
    b = c.disco_batch(3)
    c.close()
    if case["sigma"]:
        assert np.allclose(g["loc_weights"], dc.sigma_weights(case)[0], rtol=1e-6)
    b.set(L.DCB_A_MAT, np.stack([g["a_mat0"] * np.float32(0.5), g["a_mat0"], g["a_mat0"] + np.float32(0.1)]))
    b.set(L.DCB_A_SEQ, np.stack([g["a_seq0"] + np.float32(0.1), g["a_seq0"], g["a_seq0"] * np.float32(0.5)]))
    worst = {}
    for k in range(T):
        state = g["state"] if k == 0 else g["plant"][k - 1]
        states = np.stack([state + np.float32(0.1), state, state - np.float32(0.2)]).astype(np.float32)
        acts = np.stack([g["actions"][k][::-1], g["actions"][k], g["actions"][k] + np.float32(0.1)])
        rows = g["sigma_points"] if case["sigma"] else (g["params"][k] if "params" in g else None)
        params = None if rows is None else np.stack([rows * np.float32(1.02), rows, rows * np.float32(0.97)]).astype(np.float32)
        b.forward(states, acts, params, around_a_mat=True)
        fw = _records(b)
        nxt = b.step(case["strategy"], case["steps"])
        st = _records(b)
        got = dict(costs=fw["COSTS"], omega=fw["OMEGA"], a_mat1=fw["A_MAT"], a_mix=fw["A_MIX"], next=nxt, a_seq=st["A_SEQ"], a_mat=st["A_MAT"])
        for q, v in got.items():
            err = min(dc.loop_err(g, q, k, v[1]), dc.loop_err(g, q, k, v[1], g[q + "_f64"][k])) / float(g["tol_" + q][k])
            worst[q] = max(worst.get(q, 0.0), err)
        assert dc.loop_err(g, "costs", k, fw["COSTS"][0]) > 100 * float(g["tol_costs"][k])  # (the neighbours are other problems)
    b.close()
    print("%-11s " % cid + "  ".join("%s %.2f" % kv for kv in worst.items()) + "  (stored tolerances)")
    for q, v in worst.items():
        assert v < 1.0, (cid, q, v)


def _ut_pair(g, n_envs):
    import torch.distributions as dist
    from dust_amd.controllers import BatchDISCO
    from dust_amd.costs import PendulumQuadCos
    from dust_amd.models import PendulumModel
    from dust_amd.utils.utf import MerweScaledUTF

    N, H, S = int(g["N"]), int(g["H"]), int(g["S"])
    dyn = dist.Independent(dist.Uniform(torch.tensor([0.6, 0.7]), torch.tensor([1.3, 1.2])), 1)
    model = PendulumModel(length=dyn.mean[0], mass=dyn.mean[1], uncertain_params=("length", "mass"))
    cost = PendulumQuadCos()
    ctrl = BatchDISCO(n_envs, model.observation_space, model.action_space, H, N, S, temperature=0.8, a_cov=1.2 ** 2 * torch.eye(1),
                      inst_cost_fn=cost.inst_cost, term_cost_fn=cost.term_cost, params_sampling=MerweScaledUTF(n=2, alpha=0.5), params_log_space=False)
    return model, dyn, ctrl


def test_disco_ut_fixture_in_the_middle_slot(golden):
    """tests/test_gpu_mirror_api.py's sigma-point stages and tolerances, through `BatchDISCO`"""
    g = golden("disco_ut")
    model, dyn, ctrl = _ut_pair(g, 3)
    a0 = torch.tensor(g["a_mat0"])
    ctrl.a_mat = torch.stack([a0 + 0.1, a0, 0.5 * a0])
    state = torch.tensor(g["state"])
    states = torch.stack([state + 0.1, state, state - 0.2])
    acts = torch.tensor(g["actions"])
    costs, omega = ctrl.forward(states, model, dyn, ext_actions=torch.stack([acts.flip(0), acts, acts + 0.1]))
    assert elemerr(costs[1].numpy(), g["costs"]) < 1e-5
    wtol = 8 * float(np.spacing(np.float32(np.abs(g["costs"]).max()))) / 0.8
    assert relerr(omega[1].numpy(), g["omega"]) < wtol
    assert relerr(ctrl.a_mix[1].numpy(), g["a_mix"]) < wtol
    assert elemerr(costs[0].numpy(), g["costs"]) > 1e-3
    a1 = torch.tensor(g["a_mat1"])
    ctrl.a_mat = torch.stack([a1, a1, a1])
    ext = torch.tensor(g["ext_actions"])
    costs2, omega2 = ctrl.forward(states, model, dyn, ext_actions=torch.stack([ext, ext, ext]))
    assert elemerr(costs2[1].numpy(), g["costs_ext"]) < 1e-5 and relerr(omega2[1].numpy(), g["omega_ext"]) < wtol


# ------------------------------------------------------------------------------------------------ 6. plumbing
def test_one_launch_per_call_and_refusals_before_any_launch():
    L = _L()
    case = dc.BY_ID["multi_avg"]
    inp, B, H = dc.inputs(case), case["B"], case["H"]
    b = _batch(case, inp)
    b.ctx.profile(True)
    total = lambda: sum(v[1] for v in b.ctx.profile_get().values())
    b.forward(inp["states"], None, inp["params"])
    assert total() == 1
    b.step("average", 1)
    assert total() == 2
    b.tick(inp["states"], "argmax", 2, params=inp["params"])
    assert total() == 3
    assert list(b.ctx.profile_get()) == [L.load().dust_kernel_name(L.K_ROLLOUT).decode()]  # the slot of the lone forward's launch
    before = _records(b)
    lib, FP = L.load(), L.FP
    P = lambda a: None if a is None else np.ascontiguousarray(a, np.float32).ctypes.data_as(FP)
    nxt = np.zeros((B, H, 1), np.float32)
    keep = [np.ascontiguousarray(inp[k], np.float32) for k in ("states", "params", "ext")]
    st, pr, ext = (a.ctypes.data_as(FP) for a in keep)
    out = nxt.ctypes.data_as(FP)
    fwd = lambda s=st, p=pr, fl=0: lib.dust_disco_batch_forward(b._h, s, None, p, fl, None)
    stp = lambda strat=1, steps=1, e=None, o=out: lib.dust_disco_batch_step(b._h, strat, steps, e, None, o)
    tck = lambda s=st, p=pr, fl=0, strat=1, steps=1, e=None, o=out: lib.dust_disco_batch_tick(b._h, s, None, p, fl, None, strat, steps, e, o)
    refused = [(fwd(s=None), L.ERR_INVALID), (fwd(p=None), L.ERR_INVALID), (fwd(fl=L.PTR_DEVICE), L.ERR_UNSUPPORTED),
               (fwd(fl=L.STORE_STATES), L.ERR_UNSUPPORTED), (fwd(fl=L.EPS_F16), L.ERR_UNSUPPORTED), (fwd(fl=L.DISCO_PARAMS_ONCE), L.ERR_UNSUPPORTED),
               (stp(strat=3), L.ERR_INVALID), (stp(strat=-1), L.ERR_INVALID), (stp(strat=L.STEP_EXTERNAL), L.ERR_INVALID),
               (stp(steps=0), L.ERR_INVALID), (stp(steps=H + 1), L.ERR_INVALID), (stp(o=None), L.ERR_INVALID),
               (tck(s=None), L.ERR_INVALID), (tck(p=None), L.ERR_INVALID), (tck(strat=L.STEP_EXTERNAL), L.ERR_INVALID), (tck(steps=H + 1), L.ERR_INVALID),
               (tck(o=None), L.ERR_INVALID), (tck(fl=L.STORE_F16), L.ERR_UNSUPPORTED),
               (lib.dust_disco_batch_forward(None, st, None, pr, 0, None), L.ERR_INVALID),
               (lib.dust_disco_batch_set(b._h, L.DCB_A_MIX, st), L.ERR_INVALID), (lib.dust_disco_batch_get(b._h, 17, out), L.ERR_INVALID)]
    for k, (got, want) in enumerate(refused):
        assert got == want, (k, got, want)
    assert total() == 3 and not nxt.any()
    _same(_records(b), before)
    with pytest.raises(L.DustError) as e:  # the actions are kept on request only
        b.get(L.DCB_ACTIONS)
    assert e.value.status == L.ERR_STATE
    assert stp(strat=L.STEP_EXTERNAL, e=ext) == L.OK and total() == 4
    b.close()
    # dim_p = 0: no parameter rows; before a forward there is no record
    c0 = dc.BY_ID["mppi"]
    i0 = dc.inputs(c0)
    b0 = _batch(c0, i0)
    b0.ctx.profile(True)
    with pytest.raises(L.DustError) as e:
        b0.forward(i0["states"], None, np.ones((c0["B"], 1, 1), np.float32))
    assert e.value.status == L.ERR_INVALID
    with pytest.raises(L.DustError) as e:
        b0.get(L.DCB_COSTS)
    assert e.value.status == L.ERR_STATE
    assert np.array_equal(b0.get(L.DCB_A_MIX), np.ones((c0["B"], 1), np.float32))  # ones until a forward (disco.py:108)
    assert sum(v[1] for v in b0.ctx.profile_get().values()) == 0
    b0.close()


def test_create_refuses_what_lies_outside_the_box():
    from dust_amd import Context

    L = _L()
    part = dc.BY_ID["part"]
    c = _proto(part, M=3, uncertain_params=("mass",), sampling=True)
    c.set_param_weights(np.array([0.5, 0.25, 0.25], np.float32))
    with pytest.raises(L.DustError) as e:  # sigma points on Particle: the lone path has none either
        c.disco_batch(2)
    assert e.value.status == L.ERR_UNSUPPORTED
    c.close()
    skid = dc.BY_ID["skid"]
    c = _proto(skid, a_cov=((0.09, 0.03), (0.03, 0.0625)))
    with pytest.raises(L.DustError) as e:  # a full a_cov
        c.disco_batch(2)
    assert e.value.status == L.ERR_UNSUPPORTED
    c.close()
    c = Context(**dict(dc.context_kwargs(dc.BY_ID["skid_nav_sigma"])))  # the navigation cost without its map
    with pytest.raises(L.DustError) as e:
        c.disco_batch(2)
    assert e.value.status == L.ERR_STATE
    c.close()
    cart = dc.BY_ID["cart"]
    c = _proto(dict(cart, sigma=True, M=5), M=5, ctrl_penalty=0.5)  # sigma points with a_reg != 0 on cart-pole: the lone path's refusal
    with pytest.raises(L.DustError) as e:
        c.disco_batch(2)
    assert e.value.status == L.ERR_UNSUPPORTED
    c.close()


# ------------------------------------------------------------------------------------------------ 7. the class
def test_class_against_lone_multidisco_objects():
    """`BatchDISCO` against B `MultiDISCO` objects of this library over three periods, a deep copy of everything after the first: the
    same device-drawn actions bit for bit, the tolerances of item 4 downstream; first-divergence form"""
    import torch.distributions as dist

    B, seeds = 3, [11, 12, 13]
    model, batch, lone = _pair(B, seeds)
    pd = dist.Independent(dist.Uniform(torch.tensor([0.8, 0.8]), torch.tensor([1.2, 1.2])), 1)
    g = torch.Generator().manual_seed(5)
    a0 = 0.5 * torch.randn(B, 3, 6, 1, generator=g)
    batch.a_mat = a0
    for e in range(B):
        lone[e].a_mat = a0[e]
    assert tuple(batch.a_mat.shape) == (B, 3, 6, 1) and tuple(batch.a_mix.shape) == (B, 3) and tuple(batch.a_seq.shape) == (B, 6, 1)
    states = torch.tensor([[3.0, 0.0], [2.5, 0.2], [3.4, -0.1]])
    for t in range(3):
        params = torch.stack([pd.sample([2]) for _ in range(B)])
        costs, omega = batch.forward(states, model, pd, params=params)
        for e in range(B):
            lone[e].draw_source = type("Rows", (), dict(next_params=lambda self, p=params[e]: p, next_eps=lambda self: None,
                                                       next_ctrl_noise=lambda self: None))()
            cl, _, _, ol, _ = lone[e].forward(states[e], model, pd)
            assert elemerr(costs[e].numpy(), cl.numpy()) < COST_TOL, (t, e)
            assert elemerr(omega[e].numpy(), ol.numpy()) < EXP_TOL, (t, e)
            assert elemerr(batch.a_mat[e].numpy(), lone[e].a_mat.numpy()) < EXP_TOL, (t, e)
        strat = "average" if t % 2 == 0 else "argmax"
        nb = batch.step(strat, 2)
        for e in range(B):
            nl = lone[e].step(strat, 2)
            assert elemerr(nb[e].numpy(), nl.numpy()) < EXP_TOL, (t, e)
            assert elemerr(batch.a_mix[e].numpy(), lone[e].a_mix.numpy()) < EXP_TOL, (t, e)
        if t == 0:
            batch, lone = copy.deepcopy(batch), [copy.deepcopy(o) for o in lone]
        for e in range(B):  # first-divergence form: the lone objects take the batch's plans over
            lone[e].a_mat = batch.a_mat[e]
            lone[e].a_seq = batch.a_seq[e]
        states = states + 0.05


def test_class_tick_and_deepcopy_continue_identically():
    import torch.distributions as dist

    B, seeds = 2, [21, 22]
    model, batch, _ = _pair(B, seeds)
    pd = dist.Independent(dist.Uniform(torch.tensor([0.8, 0.8]), torch.tensor([1.2, 1.2])), 1)
    states = torch.tensor([[3.0, 0.0], [2.5, 0.2]])
    torch.manual_seed(3)
    batch.tick(states, model, pd, "average", 1)
    twin = copy.deepcopy(batch)
    torch.manual_seed(4)
    a = batch.tick(states, model, pd, "argmax", 2, active=[1, 0])
    torch.manual_seed(4)
    b = twin.tick(states, model, pd, "argmax", 2, active=[1, 0])
    assert torch.equal(a[0], b[0]) and bool(torch.isnan(a[1]).all()) and tuple(a.shape) == (B, 2, 1)
    assert torch.equal(batch.a_mat, twin.a_mat) and torch.equal(batch.a_seq, twin.a_seq) and torch.equal(batch.a_mix, twin.a_mix)
