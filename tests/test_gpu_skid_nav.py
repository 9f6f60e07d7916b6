"""The skid-steer navigation cost family on the device (csrc/skid.hpp skid_rollout_body<UT, NAV = true>, csrc/amppi.hpp
amppi_skid_nav_kernel; dust_set_obstacle_cost): the quadratic family plus w_obs * occ(x, y) on an occupancy grid, against the reference's
own MultiDISCO.forward and AMPPI.update_actions on its SkidSteerRobot with that cost as a callable (tests/golden/skid_nav_<tag>.npz,
amppi_nav_<tag>.npz, made by tests/golden/make_golden_skid_nav.py from the scenarios of tests/skid_nav_cases.py) - through the C ABI, the
mirror classes, both map paths (LDS and device memory), device-drawn noise, clones, shards, the dual loop and the example.

Every fixture tolerance is the fixture's own, measured from the reference alone; a comparison takes the smaller distance to the
reference's fp32 and float64 values.  The fixtures' inputs keep every rollout state >= 1e-4 cells from a cell edge, so the discontinuous
term is the same number in every correct evaluation.
"""
import copy

import numpy as np
import pytest

import skid_nav_cases as cases
from helpers import elemerr, relerr

pytestmark = pytest.mark.gpu
TOL = 1e-5  # the project's stage tolerance (where no fixture carries one)


def _err(got, g, q):
    """elemerr against the reference's fp32 or float64 value of quantity q, whichever is nearer"""
    return min(elemerr(got, g[q]), elemerr(got, cases.twin(g, q)))


def _ctx(s, g, **kw):
    from dust_amd import Context

    c = Context(grid=cases.unpack_map(g), **cases.context_kwargs(s, **kw))
    if "loc_weights" in g:
        c.set_param_weights(g["loc_weights"])
    return c


def _params(s, g):
    return g["sigma_points"] if "sigma_points" in g else (g["params"] if "params" in g else None)


def _forward(c, s, g, mode):
    """one MultiDISCO.forward on the context from the recorded actions, or one likelihood sample from the recorded eps -> dict of quantities"""
    c.set_a_mat(g["a_mat0"])
    c.set_a_seq(g["a_seq0"])
    params = _params(s, g)
    if mode == "actions":
        costs, states, _, omega = c.disco_forward(g["state"], g["ext_actions"], params=params, want_states=True)
        return dict(costs=costs, states=states, omega=omega, a_mat1=c.get_a_mat(), a_mix=c.get_a_mix())
    c.set_theta(g["a_mat0"])
    costs, actions = c.likelihood_sample(g["state"], g["eps"], params, want_actions=True)
    assert np.array_equal(actions, g["ext_actions"]), "theta + L eps must be bit-exact"
    assert np.array_equal(c.get_costs(), costs)
    return dict(costs=costs, a_mat1=c.get_a_mat(), a_mix=c.get_a_mix())


def _amppi(c, s, g, **kw):
    c.set_a_seq(g["a_seq0"])
    costs, omega, a_seq, states, _ = c.amppi_update(g["state"], g["actions"], _params(s, g), shared_params=s["mode"] == "single", want_states=True, **kw)
    return dict(costs=costs, omega=omega, a_seq1=a_seq, states=states)


def _check(name, got, g, s):
    errs = {q: _err(v, g, q) for q, v in got.items()}
    print(name + "  " + "  ".join("%s %.1e/%.1e" % (q, e, float(g["tol_" + q])) for q, e in errs.items()))
    for q, e in errs.items():
        assert e < float(g["tol_" + q]), (name, q, e, float(g["tol_" + q]))
    for v in s["offs"]:  # held AWAY from every variant: the reference is >= 10 tolerances from it (test_skid_nav_cpu.py), the device >= 5
        assert elemerr(g["costs_off_" + v], got["costs"]) >= 5 * float(g["tol_costs"]), (name, v)


# ------------------------------------------------------------------------------------------------ 1. the fixtures through the Context
@pytest.mark.parametrize("mode", ["actions", "eps"])
@pytest.mark.parametrize("name", cases.ROLLOUT_NAMES)
def test_rollout_fixtures_vs_reference(golden, name, mode):
    """skid_nav_rollout_kernel / skid_ut_nav_rollout_kernel + the regular kernel's second pass against the reference's MultiDISCO.forward
    with the navigation cost: costs, every rollout's states, omega, the a_mat update and a_mix from recorded actions; costs, the a_mat
    update and a_mix from recorded eps (the device forms theta + L eps itself, bit for bit).  `bigmap` (5000 words) reads the map from
    device memory, every other fixture from LDS."""
    s = cases.ROLLOUT_BY_TAG[name]
    g = golden(cases.fixture_name(s))
    c = _ctx(s, g)
    got = _forward(c, s, g, mode)
    c.close()
    _check("%s [%s]" % (name, mode), got, g, s)


@pytest.mark.parametrize("name", cases.AMPPI_NAMES)
def test_amppi_fixtures_vs_reference(golden, name):
    """amppi_skid_nav_kernel against the reference's AMPPI.update_actions with the navigation cost, from the recorded actions (the C entry
    takes actions, not eps: the fixture's actions ARE a_seq0 + L eps of its recorded eps, asserted): costs, omega, the updated sequence and
    the trajectories"""
    s = cases.AMPPI_BY_TAG[name]
    g = golden(cases.fixture_name(s))
    assert np.array_equal(cases.actions_of(s, g["a_seq0"][None], g["eps"]), g["actions"])
    c = _ctx(s, g)
    got = _amppi(c, s, g)
    assert np.array_equal(c.get_a_seq(), got["a_seq1"])
    c.close()
    _check(name, got, g, s)


@pytest.mark.parametrize("name", ["nominal", "ut_p1", "amppi:wave", "amppi:ut_p2"])
def test_both_map_paths_are_bit_identical(golden, name, monkeypatch):
    """The same small-map fixture with the map staged into LDS (the default up to 4096 words) and read from device memory (the development
    switch DUST_NAV_GRID_HBM=1, read once when the context is created): the same bits, and the reference's numbers on either path"""
    amppi = name.startswith("amppi:")
    s = (cases.AMPPI_BY_TAG if amppi else cases.ROLLOUT_BY_TAG)[name.split(":")[-1]]
    g = golden(cases.fixture_name(s))
    run = (lambda c: _amppi(c, s, g)) if amppi else (lambda c: _forward(c, s, g, "actions"))
    lds = _ctx(s, g)
    monkeypatch.setenv("DUST_NAV_GRID_HBM", "1")
    hbm = _ctx(s, g)
    monkeypatch.delenv("DUST_NAV_GRID_HBM")
    a, b = run(lds), run(hbm)  # (the switch was read at creation: deleting it changes nothing for `hbm`)
    lds.close(); hbm.close()
    for q in a:
        assert np.array_equal(a[q], b[q]), q
    _check(name + " [device memory]", b, g, s)


# ------------------------------------------------------------------------------------------------ 2. the mirror classes
def _nav_cost(s, g):
    import torch

    from dust_amd.costs import NavigationCost
    from dust_amd.utils.obstacle_map import ObstacleMap

    om = ObstacleMap(list(s["map_dim"]), s["cell"])
    om.map = cases.unpack_map(g).astype(np.float64)
    wc = torch.tensor(s["w_ctrl"]) if any(s["w_ctrl"]) else None
    return NavigationCost(cases.GOAL, cases.W_STATE, cases.W_TERM, wc, obst_map=om, w_obs=s["w_obs"])


def _model(s):
    from dust_amd.models import SkidSteerRobot

    return SkidSteerRobot(delta_t=s["dt"], uncertain_params=s["up"] or None, min_wheel_speed=s["bounds"][0], max_wheel_speed=s["bounds"][1], **s["fixed"])


@pytest.mark.parametrize("name", ["areg", "ut_p1"])
def test_multidisco_with_a_navigation_cost(golden, name):
    """MultiDISCO(inst_cost_fn=NavigationCost(...).inst_cost, ...).forward: the class hands the cost's map, cell size and w_obs to the
    device with everything else (ctrl_penalty, a_seq, the dynamics samples / the sigma points); a changed map rebuilds the context"""
    import torch
    import torch.distributions as dist

    from dust_amd.controllers import MultiDISCO
    from dust_amd.utils.utf import MerweScaledUTF
    from helpers import RecordedDraws

    s = cases.ROLLOUT_BY_TAG[name]
    g = golden(cases.fixture_name(s))
    model, cost = _model(s), _nav_cost(s, g)
    ut = s["kind"] == "ut"
    ctrl = MultiDISCO(model.observation_space, model.action_space, s["H"], s["N"], s["S"], temperature=cases.TEMPERATURE, ctrl_penalty=s["ctrl_penalty"],
                      a_cov=torch.tensor(cases.a_cov_of(s), dtype=torch.float), inst_cost_fn=cost.inst_cost, term_cost_fn=cost.term_cost,
                      params_sampling=MerweScaledUTF(n=len(s["up"]), alpha=float(g["alpha"])) if ut else True, params_samples=s["M"],
                      params_log_space=s["log"])
    ctrl.a_mat = torch.tensor(g["a_mat0"])
    ctrl.a_seq = torch.tensor(g["a_seq0"])
    if ut:
        pdist = dist.MultivariateNormal(torch.tensor(g["dist_mean"]), covariance_matrix=torch.diag(torch.tensor(g["dist_std"]) ** 2))
    else:
        pdist = dist.Independent(dist.Uniform(torch.tensor(s["lo"]), torch.tensor(s["hi"])), 1)
        ctrl.draw_source = RecordedDraws(params=[g["params"]])
    costs, states, _, omega, _ = ctrl.forward(torch.tensor(g["state"]), model, pdist, ext_actions=torch.tensor(g["ext_actions"]))
    got = dict(costs=costs.numpy(), states=states.numpy(), omega=omega.numpy(), a_mat1=ctrl.a_mat.numpy(), a_mix=ctrl.a_mix.numpy())
    _check(name + " [mirror]", got, g, s)
    # a deep copy carries the map and the weight (dust_clone); a changed map is a new context and other costs
    twin = copy.deepcopy(ctrl)
    for k in (ctrl, twin):
        k.a_mat = torch.tensor(g["a_mat0"])
        if not ut:
            k.draw_source = RecordedDraws(params=[g["params"]])
    c1 = ctrl.forward(torch.tensor(g["state"]), model, pdist, ext_actions=torch.tensor(g["ext_actions"]))[0]
    c2 = twin.forward(torch.tensor(g["state"]), model, pdist, ext_actions=torch.tensor(g["ext_actions"]))[0]
    assert torch.equal(c1, c2) and np.array_equal(c1.numpy(), got["costs"])
    old = ctrl._ctx
    cost.obst_map.map = cost.obst_map.map.T.copy()
    cost.obst_map.convert_map()
    ctrl.a_mat = torch.tensor(g["a_mat0"])
    if not ut:
        ctrl.draw_source = RecordedDraws(params=[g["params"]])
    c3 = ctrl.forward(torch.tensor(g["state"]), model, pdist, ext_actions=torch.tensor(g["ext_actions"]))[0]
    assert ctrl._ctx is not old
    assert elemerr(c3.numpy(), g["costs_off_transpose"]) < float(g["tol_costs"])


def test_amppi_with_a_navigation_cost(golden):
    """AMPPI(inst_cost_fn=NavigationCost(...).inst_cost, ...).update_actions on the `extended` fixture (a full a_cov, one row per trajectory)"""
    import torch

    from dust_amd.controllers import AMPPI

    s = cases.AMPPI_BY_TAG["extended"]
    g = golden(cases.fixture_name(s))
    model, cost = _model(s), _nav_cost(s, g)
    ctrl = AMPPI(model.observation_space, model.action_space, s["H"], s["S"], lambda_=cases.TEMPERATURE, a_cov=torch.tensor(cases.a_cov_of(s), dtype=torch.float),
                 inst_cost_fn=cost.inst_cost, term_cost_fn=cost.term_cost, params_sampling=s["mode"], init_actions=torch.tensor(g["a_seq0"]))
    model.sample_params = lambda n, r=g["params"]: model.params_to_dict(torch.as_tensor(r)[:n])
    costs, states, _, omega = ctrl.update_actions(model, torch.tensor(g["state"]), torch.tensor(g["actions"]))
    _check("extended [mirror]", dict(costs=costs.numpy(), states=states.numpy(), omega=omega.numpy(), a_seq1=ctrl.a_seq.numpy()), g, s)


# ------------------------------------------------------------------------------------------------ 3. device-drawn noise
def test_device_noise_self_consistency():
    """N = 64, S = 32, M = 3, H = 20 with noise drawn on the device and the states stored: the host NavigationCost on the device's own
    stored states reproduces the device's costs to 1e-5.  A lane is left out only where one of its states lies within 1e-5 cells of an
    edge (there two roundings of p / cell + offset may pick different cells): 3 x 21 x 4 x 1e-5 = 0.25 % of the lanes from the geometry
    alone, at most 1 % asserted."""
    import torch

    from dust_amd import Context

    N, S, M, H = 64, 32, 3, 20
    s = dict(cases.ROLLOUT_BY_TAG["fullcov"], N=N, S=S, M=M, H=H, a_cov=None)
    grid = cases.make_map(s)
    rng = np.random.default_rng(41)
    th = (s["fwd"] + 0.5 * rng.standard_normal((N, H, 2))).astype(np.float32)
    params = rng.uniform(s["lo"], s["hi"], (M, 2)).astype(np.float32)
    state = np.array(s["state0"], np.float32)
    c = Context(grid=grid, **cases.context_kwargs(s, seed=7))
    c.set_theta(th); c.set_a_mat(th)
    costs, states, actions, _ = c.disco_forward(state, None, params=params, want_states=True, want_actions=True)
    c.close()
    assert states.shape == (M, S, N, H + 1, 5) and np.isfinite(states).all()
    g = dict(map_bits=cases.pack_map(grid), map_shape=np.array(grid.shape))
    cost = _nav_cost(s, g)
    st = torch.from_numpy(states)
    acts = torch.from_numpy(actions)[None].expand(M, -1, -1, -1, -1)
    inst = cost.inst_cost(st[..., :-1, :], acts).double().sum(-1)
    term = cost.term_cost(st[..., -1, :]).double()
    host = (inst + term).mean(0).numpy()
    sc = cases.scaled64(states[..., 0:2], s, grid.shape)
    near = (np.abs(sc - np.round(sc)) < 1e-5).any(axis=(0, 3, 4))  # [S, N]: some state of the lane's M rollouts on an edge
    assert near.mean() <= 0.01, near.mean()
    keep = ~near
    floor = float(np.sqrt(np.mean(host ** 2)))
    e = float((np.abs(costs[keep] - host[keep]) / (np.abs(host[keep]) + floor)).max())
    hit = float(cases.occupancy(grid, sc).mean())
    print("device noise: costs %.1e on %d of %d lanes, colliding steps %.0f %%" % (e, keep.sum(), keep.size, 100 * hit))
    assert 0.05 < hit < 0.95 and e < TOL, e


# ------------------------------------------------------------------------------------------------ 4. switching, clones
def test_w_obs_zero_returns_to_the_plain_kernels(golden):
    """set_obstacle_cost(0) after a weight > 0 gives the bits of a context that never had the term (and never saw a map)"""
    from dust_amd import Context

    s = cases.ROLLOUT_BY_TAG["ragged"]
    g = golden(cases.fixture_name(s))
    kw = cases.context_kwargs(s)
    kw.pop("w_obs")
    plain = Context(**kw)
    nav = _ctx(s, g)
    a = _forward(plain, s, g, "actions")
    b = _forward(nav, s, g, "actions")
    assert elemerr(b["costs"], a["costs"]) > 100 * TOL
    assert elemerr(a["costs"], g["costs_off_w0"]) < float(g["tol_costs"])
    nav.set_obstacle_cost(0.0)
    b0 = _forward(nav, s, g, "actions")
    for q in a:
        assert np.array_equal(a[q], b0[q]), q
    nav.set_obstacle_cost(s["w_obs"])
    b1 = _forward(nav, s, g, "actions")
    for q in b:
        assert np.array_equal(b[q], b1[q]), q
    plain.close(); nav.close()


@pytest.mark.parametrize("name", ["nominal", "amppi:wave"])
def test_clone_carries_map_and_weight(golden, name):
    amppi = name.startswith("amppi:")
    s = (cases.AMPPI_BY_TAG if amppi else cases.ROLLOUT_BY_TAG)[name.split(":")[-1]]
    g = golden(cases.fixture_name(s))
    run = (lambda c: _amppi(c, s, g)) if amppi else (lambda c: _forward(c, s, g, "actions"))
    c = _ctx(s, g)
    twin = copy.deepcopy(c)
    a = run(c)
    c.close()
    b = run(twin)
    twin.close()
    for q in a:
        assert np.array_equal(a[q], b[q]), q
    _check(name + " [clone]", b, g, s)


# ------------------------------------------------------------------------------------------------ 5. sharding
def test_sharded_equals_unsharded_with_the_navigation_cost():
    """World 2 equals unsharded (the criterion and bounds of test_sharded_equals_unsharded_with_ctrl_penalty): the shards receive the map
    and w_obs through their configuration as they receive Particle's grid"""
    from dust_amd import Context
    from dust_amd.parallel import DeviceShard, LocalComm, tick

    N, S, H, M, K, T = 64, 32, 10, 3, 2, 2
    s = dict(cases.ROLLOUT_BY_TAG["areg"], N=N, S=S, H=H, M=M)
    grid = cases.make_map(s)
    kw = dict(cases.context_kwargs(s, kernel="K1", lr=0.05, alpha=0.1, temperature=10.0, seed=11), grid=grid)
    rng = np.random.default_rng(5)
    state = np.array(s["state0"], np.float32)
    mu = (s["fwd"] + 0.4 * rng.standard_normal((N, H, 2))).astype(np.float32)
    th = (mu + 0.2 * rng.standard_normal((N, H, 2))).astype(np.float32)
    eps = rng.standard_normal((T, K, S, N, H, 2)).astype(np.float32)
    params = np.stack([[rng.uniform(s["lo"], s["hi"], (M, 2)) for _ in range(K)] for _ in range(T)]).astype(np.float32)
    ref = Context(**kw)
    ref.set_theta(th); ref.set_prior(mu); ref.set_a_mat(th)
    outs = [ref.svmpc_tick(state, K, eps[t], params[t]) for t in range(T)]
    rt = ref.get_theta()
    nav_costs = ref.get_costs()
    ref.set_obstacle_cost(0.0)
    ref.likelihood_sample(state, eps[0, 0], params[0, 0])
    assert elemerr(ref.get_costs(), nav_costs) > 100 * TOL  # (the term is there)
    shards = tuple(DeviceShard(dict(kw), r, 2) for r in range(2))
    for sh in shards:
        sh.set_state(th, mu, th)
    for t in range(T):
        a_seq, pw = tick(shards, LocalComm(), state, K, eps[t], params[t], want_outputs=True, final_gather=True)
        assert np.array_equal(a_seq, outs[t][0]), t
        assert relerr(pw, outs[t][1]) < 1e-5
    for sh in shards:
        sh.sync()
        assert elemerr(sh.ctx.get_theta(), rt) < 2e-6, sh.rank
        sh.ctx.close()
    ref.close()


# ------------------------------------------------------------------------------------------------ 6. the dual loop
def test_dual_tick_with_the_navigation_cost_equals_its_pieces():
    """dust_dual_tick on a skid-steer controller with the obstacle term against the same pieces called one by one with the same Philox
    key, three control periods: bit-identical (the pattern of test_dual_tick_on_skid_steer_equals_its_pieces)"""
    from dust_amd import Context, MpfContext
    from mpf_skid_cases import NAMES3, particles
    from test_gpu_mpf_skid import _plant

    N, S, M, H, K, Mp = 32, 16, 3, 8, 2, 130
    s = cases.ROLLOUT_BY_TAG["nominal"]
    grid = cases.make_map(s)
    rng = np.random.default_rng(11)
    mu = (0.3 + 0.2 * rng.standard_normal((N, H, 2))).astype(np.float32)
    th = (mu + 0.1 * rng.standard_normal((N, H, 2))).astype(np.float32)
    x0 = particles(NAMES3, Mp, True, 77, 0.2)
    s0 = np.array(s["state0"], np.float32)

    def make(w_obs):
        c = Context(model="skid_steer", N=N, S=S, M=M, H=H, dt=0.1, kernel="K1", lr=0.05, alpha=0.5, sigma_a=0.3, sigma_p=0.3, uncertain_params=NAMES3,
                    params_log_space=True, goal=cases.GOAL, w_quad_ctrl=(0.1, 0.1), seed=5, grid=grid, w_obs=w_obs, cell_size=s["cell"])
        c.set_theta(th); c.set_prior(mu); c.set_a_mat(th)
        m = MpfContext(x0, s0, model="skid_steer", uncertain_params=NAMES3, log_space=True, obs_std=0.05, lr=1e-4, init_bw=0.3, dt=0.1)
        return c, m

    ca, ma = make(s["w_obs"])
    cb, mb = make(s["w_obs"])
    cz, mz = make(0.0)
    sa = sb = s0
    prev = None
    for t in range(3):
        a1, p1, bw1 = ca.dual_tick(ma, sa, prev, K, mpf_steps=6, mpf_bw=None, seed=100 + t)
        if prev is not None:
            bw2 = mb.silverman()
            mb.optimize(prev, sb, bw2, 6)
            assert bw1 == bw2
        params = mb.prior_sample(K * M, 100 + t).reshape(K, M, 3)
        a2, p2 = cb.svmpc_tick(sb, K, None, params)
        assert np.isfinite(a1).all() and abs(float(p1.sum()) - 1.0) < 1e-4
        assert np.array_equal(a1, a2) and np.array_equal(p1, p2), t
        assert np.array_equal(ma.get_particles(), mb.get_particles()), t
        if t == 0:
            az, pz, _ = cz.dual_tick(mz, sa, None, K, mpf_steps=6, mpf_bw=None, seed=100)
            assert not np.array_equal(pz, p1)  # (the term is there)
        prev = a1[0].copy()
        sa = sb = _plant(sa, a1[0])
    assert np.array_equal(ca.get_theta(), cb.get_theta())
    for o in (ca, cb, cz, ma, mb, mz):
        o.close()


def test_dual_svmpc_with_the_navigation_cost_fused_equals_unfused():
    """DualSVMPC over SkidSteerRobot with a NavigationCost, five control periods: fused (one C call per period) and unfused give the same
    actions, weights and filter particles (the pattern of test_dual_svmpc_on_skid_steer_fused_equals_unfused)"""
    import torch

    from dust_amd.controllers import DualSVMPC, MultiDISCO
    from dust_amd.inference import MPF, SVMPC, ExponentiatedUtility, GaussianLikelihood, get_gmm
    from dust_amd.kernels import RBFKernel
    from dust_amd.models import SkidSteerRobot
    from mpf_skid_cases import NAMES3, particles
    from test_gpu_mpf_skid import _plant

    N, S, M, H, Mp = 16, 16, 3, 6, 130
    s = cases.ROLLOUT_BY_TAG["nominal"]
    g = dict(map_bits=cases.pack_map(cases.make_map(s)), map_shape=np.array(cases.map_cells(s)))
    rng = np.random.default_rng(21)
    mu0 = torch.tensor((0.3 + 0.2 * rng.standard_normal((N, H, 2))).astype(np.float32))
    init_policies = mu0 + torch.tensor((0.1 * rng.standard_normal((N, H, 2))).astype(np.float32))
    x0 = torch.tensor(particles(NAMES3, Mp, True, 78, 0.2))
    init_state = torch.tensor(s["state0"])
    cost = _nav_cost(dict(s, w_ctrl=(0.1, 0.1)), g)

    def make(fused):
        model = SkidSteerRobot(delta_t=0.1, uncertain_params=NAMES3)
        ctrl = MultiDISCO(observation_space=model.observation_space, action_space=model.action_space, hz_len=H, action_samples=S, params_samples=M,
                          temperature=2.0, a_cov=0.09 * torch.eye(2), inst_cost_fn=cost.inst_cost, term_cost_fn=cost.term_cost, params_sampling=True,
                          n_policies=N, params_log_space=True, seed=5)
        ctrl.a_mat = init_policies.clone()
        ctrl.return_rollouts = False
        mpf = MPF(init_particles=x0.clone(), likelihood=GaussianLikelihood(initial_obs=init_state, obs_std=0.05, model=model, log_space=True),
                  optimizer_class=torch.optim.SGD, lr=1e-4, bw=0.3, bw_scale=1.0)
        sv = SVMPC(likelihood=ExponentiatedUtility(alpha=0.5, n_samples=S, controller=ctrl, model=model), init_particles=init_policies.clone(),
                   prior=get_gmm(mu0, torch.ones(N), 0.09 * torch.eye(2)), kernel=RBFKernel(), n_particles=N, bw_scale=1.0, n_steps=1,
                   optimizer_class=torch.optim.SGD, lr=0.05)
        return DualSVMPC(sv, mpf, mpf_bw=0.3, mpf_steps=6, warm_up=0, fused=fused, seed=0)

    def plant(state, action):
        return torch.from_numpy(_plant(state.reshape(-1).numpy(), action.reshape(-1).numpy())).reshape(1, -1)

    fu, un = make(True), make(False)
    sf = su = init_state.reshape(1, -1)
    for t in range(5):
        af, sf, pf = fu.tick(sf, plant)
        au, su, pu = un.tick(su, plant)
        assert torch.isfinite(af).all() and abs(float(pf.sum()) - 1.0) < 1e-4, t
        assert torch.equal(af, au) and torch.equal(pf, pu) and torch.equal(sf, su), t
    assert fu._pending is not None and un._pending is None
    assert torch.equal(fu.dyn_particles, un.dyn_particles) and not torch.equal(un.dyn_particles, x0)
    assert torch.equal(fu.theta, un.theta)
    assert float(fu.controller._ctx.cfg.cell_size) == pytest.approx(s["cell"])


# ------------------------------------------------------------------------------------------------ 7. refusals
def test_refusals(golden):
    from dust_amd import Context, _lib as L

    s = cases.ROLLOUT_BY_TAG["nominal"]
    g = golden(cases.fixture_name(s))
    # no grid: DUST_ERR_STATE at the first rollout, with the Particle family's wording
    c = Context(**cases.context_kwargs(s))
    c.set_a_mat(g["a_mat0"])
    with pytest.raises(L.DustError, match="no occupancy grid was supplied") as e:
        c.disco_forward(g["state"], g["ext_actions"])
    assert e.value.status == L.ERR_STATE
    c.set_grid(cases.unpack_map(g))
    assert _err(c.disco_forward(g["state"], g["ext_actions"])[0], g, "costs") < float(g["tol_costs"])
    for bad in (-1.0, float("nan"), float("inf")):
        with pytest.raises(L.DustError) as e:
            c.set_obstacle_cost(bad)
        assert e.value.status == L.ERR_INVALID
    with pytest.raises(L.DustError) as e:  # a non-binary map: the library's existing refusal
        c.set_grid(0.5 * cases.unpack_map(g))
    assert e.value.status == L.ERR_UNSUPPORTED
    c.close()
    # a configuration without a cell size: the lookups scale by 1 / cell_size, so the weight is refused (0 stays allowed)
    for cell in (0.0, -0.1, float("nan")):
        kw = dict(cases.context_kwargs(s), cell_size=cell)
        kw.pop("w_obs")
        c = Context(**kw)
        with pytest.raises(L.DustError, match="cell_size") as e:
            c.set_obstacle_cost(s["w_obs"])
        assert e.value.status == L.ERR_INVALID
        c.set_obstacle_cost(0.0)
        c.close()
    a = cases.AMPPI_BY_TAG["wave"]
    ga = golden(cases.fixture_name(a))
    c = Context(**cases.context_kwargs(a))
    with pytest.raises(L.DustError, match="no occupancy grid was supplied") as e:
        c.amppi_update(ga["state"], ga["actions"])
    assert e.value.status == L.ERR_STATE
    c.close()
    # the other models: Particle carries w_obs in its configuration, the Pendulum and the cart-pole have no position plane
    for kw in (dict(model="pendulum"), dict(model="particle", with_obstacle=False), dict(model="cartpole")):
        c = Context(N=2, S=4, H=3, **kw)
        with pytest.raises(L.DustError) as e:
            c.set_obstacle_cost(1.0)
        assert e.value.status == L.ERR_UNSUPPORTED
        c.close()
    # the refusals the family already has stay: sigma-point weights with a control weight, binary16 storage
    u = cases.ROLLOUT_BY_TAG["ut_p1"]
    gu = golden(cases.fixture_name(u))
    c = _ctx(u, gu, w_quad_ctrl=(0.1, 0.1))
    c.set_a_mat(gu["a_mat0"])
    with pytest.raises(L.DustError, match="sigma-point weights with a non-zero control weight") as e:
        c.disco_forward(gu["state"], gu["ext_actions"], params=gu["sigma_points"])
    assert e.value.status == L.ERR_UNSUPPORTED
    c.close()
    c = _ctx(s, g)
    c.set_a_mat(g["a_mat0"])
    with pytest.raises(L.DustError, match="binary16") as e:
        c.disco_forward(g["state"], g["ext_actions"].astype(np.float16))
    assert e.value.status == L.ERR_UNSUPPORTED
    c.close()


def test_amppi_class_refuses_a_control_weight(golden):
    import torch

    from dust_amd.controllers import AMPPI

    s = cases.AMPPI_BY_TAG["wave"]
    g = golden(cases.fixture_name(s))
    model, cost = _model(s), _nav_cost(dict(s, w_ctrl=(0.1, 0.1)), g)
    ctrl = AMPPI(model.observation_space, model.action_space, s["H"], s["S"], lambda_=cases.TEMPERATURE, a_cov=torch.eye(2), inst_cost_fn=cost.inst_cost,
                 term_cost_fn=cost.term_cost, params_sampling="none", init_actions=torch.tensor(g["a_seq0"]))
    with pytest.raises(NotImplementedError, match="amppi.py:205"):
        ctrl.update_actions(model, torch.tensor(g["state"]), torch.tensor(g["actions"]))


# ------------------------------------------------------------------------------------------------ 8. the example
def test_example_runs_at_a_tiny_size():
    import importlib.util
    import os

    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples", "skid_steer_example.py")
    spec = importlib.util.spec_from_file_location("skid_steer_example", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    states = mod.main(["--horizon", "6", "--ticks", "4", "--particles", "4", "--samples", "8", "--params", "2", "--mpf-particles", "16"])
    assert tuple(states.shape) == (5, 5) and bool(np.isfinite(states.numpy()).all())
    assert not np.array_equal(states[0].numpy(), states[-1].numpy())
