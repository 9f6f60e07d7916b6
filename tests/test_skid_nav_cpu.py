"""The skid-steer navigation fixtures (tests/golden/skid_nav_<tag>.npz, amppi_nav_<tag>.npz, made by tests/golden/make_golden_skid_nav.py from
the scenarios of tests/skid_nav_cases.py) and the host side of the navigation cost family, without a GPU: the float64 restatement of
rollout + cost reproduces every `_f64` twin to 1e-12; the conditions the generator stored hold (edge margin, stable cells, collision
share, power, caps, sizes); dust_amd.costs.NavigationCost is bit-equal to the reference's Particle-style expression on the recorded
states; dust_set_obstacle_cost is exported and bound; recognise() returns the obstacle weight and refuses what would drop it; the new
kernel instances spill nothing.
"""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import __graft_entry__ as entry
import skid_nav_cases as cases
from helpers import elemerr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALL = cases.ROLLOUTS + cases.AMPPI
IDS = [cases.fixture_name(s) for s in ALL]


@pytest.fixture(scope="module")
def built():
    return entry.build()


# ---------------------------------------------------------------------------------------------- the fixtures
@pytest.mark.parametrize("s", ALL, ids=IDS)
def test_float64_restatement_matches_the_twins(golden, s):
    """skid_nav_cases.restate_disco / restate_amppi - SkidSteerRobot.step, the quadratic cost and w_obs * get_collisions in float64 numpy,
    combined as the controller combines them - against every `_f64` twin to 1e-12"""
    g = golden(cases.fixture_name(s))
    grid = cases.unpack_map(g)
    r = (cases.restate_amppi if s["kind"] == "amppi" else cases.restate_disco)(s, g, grid)
    for q in (cases.AMPPI_QUANT if s["kind"] == "amppi" else cases.ROLLOUT_QUANT):
        t64 = cases.twin(g, q)
        assert t64.dtype == np.float64 and t64.shape == g[q].shape
        e = elemerr(r[q], t64)
        assert e < 1e-12, (q, e)


@pytest.mark.parametrize("s", ALL, ids=IDS)
def test_fixture_conditions_hold(golden, s):
    """What the generator asserted and stored, recomputed from the stored arrays: the map is the scenario's, the edge margin (>= 1e-4 cells
    and >= 10 x the fp32 - float64 difference of the scaled position), the same cell in the fp32 and the float64 run, the collision share in
    [5 %, 95 %], every `_off` variant >= 10 tolerances away, 1e-5 <= tol <= 5e-5 with 2 d <= tol, the seed within 500 tries, the file
    under 512 KiB, <= 5 000 lane-steps"""
    name = cases.fixture_name(s)
    g = golden(name)
    grid = cases.unpack_map(g)
    assert np.array_equal(grid, cases.make_map(s)) and set(np.unique(grid)) <= {0.0, 1.0}
    assert g["map_bits"].dtype == np.uint8 and g["map_bits"].size == (grid.size + 7) // 8
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", name + ".npz")) < 512 * 1024
    assert 1 <= int(g["tries"]) <= cases.MAX_TRIES and int(g["seed"]) == s["seed"] + int(g["tries"]) - 1
    st = g["states"]
    assert st.shape[:-2] == ((s["M"], s["S"], s["N"]) if s["kind"] != "amppi" else (s["S"] * (2 * len(s["up"]) + 1 if s["mode"] == "ut" else 1),))
    assert s["S"] * s["N"] * s["H"] <= 5000  # (lanes x steps)
    sc32 = cases.scaled32(st[..., 0:2], s, grid.shape)
    sc64 = cases.scaled64(cases.twin(g, "states")[..., 0:2], s, grid.shape)
    margin = float(np.abs(sc32.astype(np.float64) - np.round(sc32)).min())
    diff = float(np.abs(sc32.astype(np.float64) - sc64).max())
    assert margin == float(g["margin"]) >= cases.MARGIN and abs(diff - float(g["scaled_diff"])) < 1e-12
    assert margin >= cases.MARGIN_RATIO * diff, (margin, diff)
    assert bool(g["stable_cells"]) and np.array_equal(np.floor(sc32).astype(np.int64), np.floor(sc64).astype(np.int64))
    share = float(cases.occupancy(grid, cases.scaled64(st[..., 0:2], s, grid.shape)).mean())
    assert abs(share - float(g["collision_share"])) < 1e-12 and 0.05 <= share <= 0.95
    for q in (cases.AMPPI_QUANT if s["kind"] == "amppi" else cases.ROLLOUT_QUANT):
        tol = float(g["tol_" + q])
        assert cases.TOL <= tol <= cases.CAP and 2.0 * elemerr(g[q], cases.twin(g, q)) <= tol * (1 + 1e-12) + 1e-12, q
    for v in s["offs"]:
        off = cases.costs_off(s, g, grid, v)
        assert np.array_equal(off, g["costs_off_" + v])
        assert elemerr(off, g["costs"]) >= 10 * float(g["tol_costs"]), v
    assert not [k for k in g if k.startswith("costs_off_") and k[10:] not in s["offs"]]
    if "free" in s["offs"]:  # the trajectories leave the map on both sides of both axes
        assert sc64[..., 0].min() < 0 and sc64[..., 0].max() >= grid.shape[0] and sc64[..., 1].min() < 0 and sc64[..., 1].max() >= grid.shape[1]
        assert float(np.min(g["offmap_sides"])) > 0.005


def test_scenarios_cover_the_shapes():
    by = cases.ROLLOUT_BY_TAG
    assert by["nominal"]["N"] * by["nominal"]["S"] == 96 and not by["nominal"]["up"]
    r = by["ragged"]
    assert r["N"] * r["S"] == 333 and r["H"] * 2 == 30 and len(r["up"]) == 2
    assert len(by["p3_log"]["up"]) == 3 and by["p3_log"]["log"] and by["scalar"]["dist"] == "scalar"
    assert (by["scalar"]["N"] * by["scalar"]["S"]) % by["scalar"]["M"] != 0
    assert by["areg"]["ctrl_penalty"] == 0.6 and by["areg"]["a_seq"] and by["fullcov"]["a_cov"] is not None
    nx, ny = cases.map_cells(by["bigmap"])
    assert (nx * ny + 31) // 32 > 4096
    assert all((cases.map_cells(s)[0] * cases.map_cells(s)[1] + 31) // 32 <= 4096 for s in cases.ROLLOUTS + cases.AMPPI if s["tag"] != "bigmap")
    for t, P in (("ut_p1", 1), ("ut_p3", 3)):
        assert len(by[t]["up"]) == P and by[t]["H"] % (2 * P + 1) != 0
    a = cases.AMPPI_BY_TAG
    assert a["one"]["S"] == 1 and a["wave"]["S"] == 64 and a["odd_257"]["S"] == 257 and a["odd_257"]["H"] % 2 == 1
    assert {a[t]["mode"] for t in ("single", "extended", "ut_p2")} == {"single", "extended", "ut"} and len(a["ut_p2"]["up"]) == 2
    assert all(5.0 <= s["w_obs"] <= 20.0 and 0.05 <= s["cell"] <= 0.1 for s in cases.ROLLOUTS + cases.AMPPI)


# ---------------------------------------------------------------------------------------------- the host cost
def _host_cost(s, g, obst_map=None):
    import torch

    from dust_amd.costs import NavigationCost
    from dust_amd.utils.obstacle_map import ObstacleMap

    if obst_map is None:
        obst_map = ObstacleMap(list(s["map_dim"]), s["cell"])
        obst_map.map = cases.unpack_map(g).astype(np.float64)
    wc = None if not any(s["w_ctrl"]) else torch.tensor(s["w_ctrl"])
    return NavigationCost(cases.GOAL, cases.W_STATE, cases.W_TERM, wc, obst_map=obst_map, w_obs=s["w_obs"])


@pytest.mark.parametrize("s", ALL, ids=IDS)
def test_host_cost_is_the_reference_expression(golden, s):
    """NavigationCost.inst_cost / term_cost on the fixture's recorded states, bit for bit the expression of Particle.default_inst_cost /
    default_term_cost (particle.py:170-225: state_cost.sum(-1) + control_cost.sum(-1) + obst_cost with ObstacleMap.get_collisions,
    obstacle_map.py:64-93) written out here in torch; combined as the controller combines them (float64) they are the reference's recorded
    costs to the fixture's tolerance."""
    import torch

    g = golden(cases.fixture_name(s))
    grid = cases.unpack_map(g)
    cost = _host_cost(s, g)
    st = torch.from_numpy(g["states"])
    goal, w_state, w_term = (torch.tensor(v) for v in (cases.GOAL, cases.W_STATE, cases.W_TERM))
    gm = torch.from_numpy(grid)

    def collisions(X):
        occ = (X * (1 / s["cell"]) + torch.Tensor([int(grid.shape[0] / 2), int(grid.shape[1] / 2)])).floor().type(torch.LongTensor)
        occ[..., 0] = occ[..., 0].clamp(0, grid.shape[0] - 1)
        occ[..., 1] = occ[..., 1].clamp(0, grid.shape[1] - 1)
        return gm[occ[..., 0], occ[..., 1]]

    amppi = s["kind"] == "amppi"
    xs = st[..., 1:, :] if amppi else st[..., :-1, :]
    acts = None
    if s["kind"] == "disco":
        acts = torch.from_numpy(g["ext_actions"])[None].expand(s["M"], -1, -1, -1, -1)
    d = xs - goal
    ref_inst = (torch.mul(d, d) * w_state).sum(-1)
    if acts is not None and any(s["w_ctrl"]):
        ref_inst = ref_inst + (torch.mul(acts, acts) * torch.tensor(s["w_ctrl"])).sum(-1)
    ref_inst = ref_inst + s["w_obs"] * collisions(xs[..., 0:2])
    dT = st[..., -1, :] - goal
    ref_term = (torch.mul(dT, dT) * w_term).sum(-1) + s["w_obs"] * collisions(st[..., -1, 0:2])
    inst, term = cost.inst_cost(xs, acts), cost.term_cost(st[..., -1, :])
    assert torch.equal(inst, ref_inst) and torch.equal(term, ref_term)
    assert float(collisions(st[..., 0:2]).mean()) == pytest.approx(float(g["collision_share"]), abs=1e-6)
    # ... and they are the recorded costs
    i64, t64 = inst.double().numpy(), term.double().numpy()
    if amppi:
        pts = st.shape[0] // s["S"]
        w = cases.weights(len(s["up"]), s["alpha"])[0] if pts > 1 else None
        c = cases.combine(s, i64.reshape(s["S"], pts, -1), t64.reshape(s["S"], pts), w)
        f = lambda a: np.asarray(a, np.float64)
        c = c + cases.TEMPERATURE * np.einsum("td,std->s", f(g["a_seq0"]) @ np.linalg.inv(cases.a_cov_of(s)), f(g["actions"]) - f(g["a_seq0"])[None])
    else:
        c = cases.combine(s, i64, t64, cases.weights(len(s["up"]), float(g["alpha"]))[0] if s["kind"] == "ut" else None)
        f = lambda a: np.asarray(a, np.float64)
        a_reg = cases.TEMPERATURE * (1 - s["ctrl_penalty"])
        c = c + a_reg * np.einsum("snhd,nhd->sn", -(f(g["ext_actions"]) - f(g["a_seq0"])), f(g["a_mat0"]) @ np.linalg.inv(cases.a_cov_of(s)))
    assert elemerr(c, g["costs"]) < float(g["tol_costs"])


def test_navigation_cost_without_a_map():
    import torch

    from dust_amd.costs import NavigationCost, QuadraticCost

    x, a = torch.randn(7, 5), torch.randn(7, 2)
    q = QuadraticCost(cases.GOAL, cases.W_STATE, cases.W_TERM, cases.W_CTRL)
    n = NavigationCost(cases.GOAL, cases.W_STATE, cases.W_TERM, cases.W_CTRL)
    assert torch.equal(n.inst_cost(x, a), q.inst_cost(x, a)) and torch.equal(n.term_cost(x), q.term_cost(x))
    with pytest.raises(ValueError, match="obst_map"):
        NavigationCost(cases.GOAL, cases.W_STATE, w_obs=3.0).inst_cost(x, a)


# ---------------------------------------------------------------------------------------------- recognition
def test_recognise_returns_the_obstacle_weight(golden):
    from dust_amd.costs import QuadraticCost, cost_grid, recognise
    from dust_amd.models import SkidSteerRobot

    s = cases.ROLLOUT_BY_TAG["nominal"]
    g = golden(cases.fixture_name(s))
    cost = _host_cost(s, g)
    model = SkidSteerRobot(delta_t=s["dt"])
    r = recognise(model, cost.inst_cost, cost.term_cost)
    assert r["w_obs"] == s["w_obs"] and r["cell_size"] == s["cell"]
    assert r["goal"] == tuple(np.float32(v) for v in cases.GOAL) and r["w_quad_ctrl"] == tuple(float(np.float32(v)) for v in s["w_ctrl"])
    assert np.array_equal(cost_grid(cost.inst_cost), cases.unpack_map(g))
    q = QuadraticCost(cases.GOAL, cases.W_STATE, cases.W_TERM)
    assert "w_obs" not in recognise(model, q.inst_cost, q.term_cost) and cost_grid(q.inst_cost) is None


def test_map_key_is_kept_between_ticks_and_follows_the_map(golden, monkeypatch):
    """The controllers put NavigationCost.grid_key() into their context key on every tick: the digest of the map is taken once, again only
    for another map - reassigned, edited in place (also where the number of occupied cells stays), or reshaped"""
    import hashlib

    from dust_amd.costs import QuadraticCost, cost_grid_key

    s = cases.ROLLOUT_BY_TAG["nominal"]
    cost = _host_cost(s, golden(cases.fixture_name(s)))
    calls = []
    real = hashlib.sha1
    monkeypatch.setattr(hashlib, "sha1", lambda b: (calls.append(1), real(b))[1])
    k0 = cost_grid_key(cost.inst_cost)
    assert k0 == (cost.obst_map.map.shape, real(cost.grid().tobytes()).hexdigest())
    assert all(cost_grid_key(cost.inst_cost) == k0 for _ in range(5)) and len(calls) == 1
    i, j = np.argwhere(cost.obst_map.map == 1)[0]
    p, q = np.argwhere(cost.obst_map.map == 0)[0]
    cost.obst_map.map[i, j], cost.obst_map.map[p, q] = 0.0, 1.0  # one obstacle cell moved in place
    k1 = cost_grid_key(cost.inst_cost)
    assert k1 != k0 and len(calls) == 2 and k1[1] == real(cost.grid().tobytes()).hexdigest()
    cost.obst_map.map = cost.obst_map.map.copy()  # another array object, the same content: the digest is taken again and agrees
    assert cost_grid_key(cost.inst_cost) == k1 and len(calls) == 3
    cost.obst_map.map = cost.obst_map.map[:-2].copy()
    assert cost_grid_key(cost.inst_cost)[0] == cost.obst_map.map.shape and len(calls) == 4
    q = QuadraticCost(cases.GOAL, cases.W_STATE)
    assert cost_grid_key(q.inst_cost) is None and cost_grid_key(lambda x, a: x.sum(-1)) is None


def test_recognise_refuses_what_would_drop_the_obstacle_term(golden):
    """A subclass of QuadraticCost passed isinstance() and lost whatever it added: refused unless it is NavigationCost itself, with its own
    methods; a weight without a map; a NavigationCost on the cart-pole; mixed owners"""
    from dust_amd.costs import NavigationCost, QuadraticCost, recognise
    from dust_amd.models import CartPoleModel, SkidSteerRobot

    s = cases.ROLLOUT_BY_TAG["nominal"]
    g = golden(cases.fixture_name(s))
    model = SkidSteerRobot(delta_t=s["dt"])

    class Extra(QuadraticCost):
        def inst_cost(self, states, controls=None, n_pol=1, debug=None):
            return super().inst_cost(states, controls) + 1.0

    class Louder(NavigationCost):
        def term_cost(self, states, n_pol=1, debug=None):
            return 2 * super().term_cost(states)

    for bad in (Extra(cases.GOAL, cases.W_STATE), Louder(cases.GOAL, cases.W_STATE, obst_map=_host_cost(s, g).obst_map, w_obs=1.0)):
        with pytest.raises(NotImplementedError, match="extends QuadraticCost"):
            recognise(model, bad.inst_cost, bad.term_cost)
    nomap = NavigationCost(cases.GOAL, cases.W_STATE, w_obs=5.0)
    with pytest.raises(ValueError, match=r"particle\.py:172-175"):
        recognise(model, nomap.inst_cost, nomap.term_cost)
    neg = NavigationCost(cases.GOAL, cases.W_STATE, obst_map=_host_cost(s, g).obst_map, w_obs=-1.0)
    with pytest.raises(ValueError, match="finite"):
        recognise(model, neg.inst_cost, neg.term_cost)
    a, b = _host_cost(s, g), _host_cost(s, g)
    with pytest.raises(NotImplementedError):
        recognise(model, a.inst_cost, b.term_cost)
    cart = NavigationCost((0, 0, 0, 0), (1, 1, 1, 1), obst_map=a.obst_map, w_obs=1.0)
    with pytest.raises(NotImplementedError, match=r"particle\.py:174"):
        recognise(CartPoleModel(), cart.inst_cost, cart.term_cost)


# ---------------------------------------------------------------------------------------------- the library
def test_library_exports_and_binds_the_entry(built):
    from dust_amd import _lib
    from dust_amd.backend import Context

    lib = C.CDLL(built)
    assert hasattr(lib, "dust_set_obstacle_cost") and "dust_set_obstacle_cost" in _lib.SYMBOLS
    assert _lib.load().dust_abi_version() == _lib.ABI_VERSION == 3
    assert callable(Context.set_obstacle_cost)
    hdr = open(os.path.join(ROOT, "include", "dust_amd.h")).read()
    doc = hdr[:hdr.index("int dust_set_obstacle_cost")].rsplit("/*", 1)[1]
    assert "particle.py:170-225" in doc and "obstacle_map.py:64-93" in doc


def test_navigation_kernels_do_not_spill(built, tmp_path):
    """the method of test_amppi_kernels_do_not_spill: the gfx950 code object's metadata shows no VGPR spill and no scratch for the three
    navigation instances - and the plain instances beside them are still there"""
    import shutil

    llvm = "/opt/rocm/lib/llvm/bin"
    if not (os.path.exists(llvm + "/llvm-objdump") and os.path.exists(llvm + "/llvm-readelf")):
        pytest.skip("llvm-objdump / llvm-readelf not available")
    shutil.copy(built, str(tmp_path / "l.so"))
    subprocess.run([llvm + "/llvm-objdump", "--offloading", "l.so"], cwd=str(tmp_path), check=True, capture_output=True)
    co = [f for f in os.listdir(str(tmp_path)) if "gfx950" in f]
    assert co, "no gfx950 code object in libdust_amd.so"
    notes = "".join(subprocess.run([llvm + "/llvm-readelf", "--notes", f], cwd=str(tmp_path), check=True, capture_output=True, text=True).stdout
                    for f in co)
    kernels = {}
    for m in re.finditer(r"\.name:\s+(\S+)\n(.*?)\.wavefront_size", notes, re.S):
        blk = m.group(2)
        kernels[m.group(1)] = (int(re.search(r"\.vgpr_spill_count:\s+(\d+)", blk).group(1)),
                               int(re.search(r"\.private_segment_fixed_size:\s+(\d+)", blk).group(1)),
                               int(re.search(r"\.vgpr_count:\s+(\d+)", blk).group(1)))
    mine = {k: v for k, v in kernels.items() if "skid_nav_rollout_kernel" in k or "skid_ut_nav_rollout_kernel" in k or "amppi_skid_nav_kernel" in k}
    assert len(mine) == 3, sorted(mine)
    for k, (spill, scratch, vgprs) in mine.items():
        print(k, "vgprs", vgprs)
        assert spill == 0 and scratch == 0 and vgprs <= 128, (k, spill, scratch, vgprs)
    assert sum(1 for k in kernels if "skid_rollout_kernel" in k or "skid_ut_rollout_kernel" in k) == 2
