"""The closed-loop episode under the reference's rules (dust_svmpc_batch_simulate, csrc/svmpc_episode.hpp svb_sim_body) without a
device: the C ABI's new entry and struct, the Python layers that name them, the register allocation of the nine new kernel instances,
the refusals of `BatchSVMPC.simulate` that need no device, and what tests/test_gpu_svmpc_sim.py relies on - the forced events, the cost
check's tolerance and its distance from three wrong costs, the fp32 replicas of both stop predicates - from the float64 restatement
alone (tests/svmpc_sim_cases.py)."""
import ctypes as C
import os
import re
import shutil
import subprocess
import tempfile

import numpy as np
import pytest

import __graft_entry__ as entry
import amppi_cases as ac
import svmpc_sim_cases as cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "dust_svmpc_batch_simulate"


@pytest.fixture(scope="module")
def built():
    return entry.build()


def test_library_declares_exports_and_binds_the_entry(built):
    from dust_amd import _lib

    lib = C.CDLL(built)
    header = open(os.path.join(ROOT, "include", "dust_amd.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    assert re.search(r"\b%s\s*\(" % NAME, code), NAME + " is not declared"
    assert hasattr(lib, NAME), NAME + " is not exported"
    assert NAME in _lib.SYMBOLS, NAME + " is not bound"
    VP, FP, IP, UP = _lib.VP, _lib.FP, C.POINTER(C.c_int), C.POINTER(C.c_ubyte)
    assert _lib.SYMBOLS[NAME] == (C.c_int, [VP, FP, C.c_int, C.c_int, FP, FP, C.POINTER(_lib.EpisodeRules), C.c_int, UP, FP, FP, FP, FP, FP, IP, IP, FP])
    # the declaration's own parameter list, type by type
    decl = re.search(r"int %s\s*\((.*?)\);" % NAME, code, re.S).group(1)
    kinds = [re.sub(r"\s*\w+$", "", p.strip()) for p in decl.split(",")]
    assert kinds == ["dust_svmpc_batch *", "const float *", "int", "int", "const float *", "const float *", "const dust_episode_rules *", "int",
                     "const unsigned char *", "float *", "float *", "float *", "float *", "float *", "int *", "int *", "float *"], kinds
    assert "simulations.py:104-130" in header and "217-260" in header
    # additive: the version, the ids and the profile counters stay where they were
    assert _lib.load().dust_abi_version() == _lib.ABI_VERSION == 3 and "#define DUST_ABI_VERSION 3" in header
    assert "DUST_K_SVMPC_BATCH = 9" in code and _lib.K_SVMPC_BATCH == 9 and _lib.K_ALL == 10


def test_rules_struct_matches_header():
    """sizeof and every field offset of dust_episode_rules from a C compile against include/dust_amd.h equal the ctypes mirror's"""
    from dust_amd import _lib

    fields = [n for n, _ in _lib.EpisodeRules._fields_]
    assert fields == ["t0", "warm_up", "stop_on_crash", "goal_radius", "goal"]
    src = '#include "dust_amd.h"\n#include <stdio.h>\n#include <stddef.h>\nint main(){printf("%zu", sizeof(dust_episode_rules));\n' + \
          "".join('printf(" %%zu", offsetof(dust_episode_rules, %s));\n' % f for f in fields) + "return 0;}\n"
    with tempfile.TemporaryDirectory() as d:
        p = os.path.join(d, "p.c")
        open(p, "w").write(src)
        subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), p, "-o", os.path.join(d, "p")], check=True)
        out = subprocess.run([os.path.join(d, "p")], check=True, capture_output=True, text=True).stdout.split()
    S = _lib.EpisodeRules
    assert [int(v) for v in out] == [C.sizeof(S)] + [getattr(S, f).offset for f in fields]
    assert C.sizeof(S) == 48 and S.goal.size == 32


def test_the_python_layers_name_the_simulation():
    import dust_amd
    import dust_amd.inference as inf
    from dust_amd.utils import simulations

    assert callable(getattr(dust_amd.SvmpcBatch, "simulate", None))
    assert callable(getattr(inf.BatchSVMPC, "simulate", None)) and callable(simulations.run_particle_episodes)
    assert inf.SimResult._fields == ("states", "actions", "p_weights", "costs", "loss", "status", "n_run", "a_seq")
    for f in ("examples/particle_sweep_example.py", "tools/svmpc_sim_time.py"):
        assert os.path.exists(os.path.join(ROOT, f)), f


def test_sim_kernels_do_not_spill(built, tmp_path):
    """the gfx950 code object's metadata shows exactly 4 + 1 + 4 new instances - svmpc_sim_kernel, svmpc_skid_nav_sim_kernel and the
    row-patching svmpc_rows_sim_kernel -, each without VGPR spill or scratch and within the 256 VGPRs of a 512-lane workgroup; none is
    caught by a substring the existing tests count kernels by"""
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
        g = lambda k: int(re.search(r"\.%s:\s+(\d+)" % k, m.group(2)).group(1))
        kernels[m.group(1)] = (g("vgpr_spill_count"), g("private_segment_fixed_size"), g("vgpr_count"))
    plain = {k: v for k, v in kernels.items() if "svmpc_sim_kernel" in k}
    nav = {k: v for k, v in kernels.items() if "svmpc_skid_nav_sim_kernel" in k}
    rows = {k: v for k, v in kernels.items() if "svmpc_rows_sim_kernel" in k}
    assert len(plain) == 4 and len(nav) == 1 and len(rows) == 4, (sorted(plain), sorted(nav), sorted(rows))
    mine = dict(plain, **nav, **rows)
    assert {k: v for k, v in kernels.items() if "_sim_kernel" in k} == mine
    for k, (spill, scratch, vgprs) in mine.items():
        print(k, "spill", spill, "scratch", scratch, "vgprs", vgprs)
        assert spill == 0 and scratch == 0 and vgprs <= 256, (k, spill, scratch, vgprs)
    for old in ("svmpc_batch_kernel", "svmpc_prior_batch_kernel", "svmpc_episode_kernel", "svmpc_skid_nav_batch_kernel", "svmpc_skid_nav_prior_batch_kernel",
                "svmpc_skid_nav_episode_kernel", "svmpc_dual_period_kernel", "sweep"):
        assert not any(old in k for k in mine), old


# ------------------------------------------------------------------------------------------------ the class, no device
def _controller(family="pendulum"):
    import torch

    from dust_amd.controllers import MultiDISCO
    from dust_amd.costs import PendulumQuadCos
    from dust_amd.inference import BatchSVMPC, ExponentiatedUtility, get_gmm
    from dust_amd.models import Particle, PendulumModel

    N, H, S = 3, 6, 16
    if family == "pendulum":
        model, cost = PendulumModel(uncertain_params=("length", "mass")), PendulumQuadCos()
        fns, da, sampling = (cost.inst_cost, cost.term_cost), 1, True
    else:  # a Particle without obstacles: no map
        model = Particle(init_state=torch.zeros(4), mass=1.0)
        fns, da, sampling = (model.default_inst_cost, model.default_term_cost), 2, None
    ctrl = MultiDISCO(model.observation_space, model.action_space, H, N, S, a_cov=4.0 * torch.eye(da), inst_cost_fn=fns[0], term_cost_fn=fns[1],
                      params_sampling=sampling, params_samples=3)
    prior = get_gmm(torch.zeros(N, H, da), torch.ones(N), 4.0 * torch.eye(da))
    lik = ExponentiatedUtility(alpha=1.0, n_samples=S, controller=ctrl, model=model)
    return BatchSVMPC(3, torch.zeros(N, H, da), prior, lik, optimizer_class=torch.optim.SGD, lr=0.5), ctrl


def test_simulate_refuses_before_any_device_call():
    import torch
    import torch.distributions as dist

    from dust_amd.inference import SimResult
    from dust_amd.utils.simulations import run_particle_episodes

    pd = dist.Independent(dist.Uniform(torch.tensor([0.6, 0.6]), torch.tensor([1.3, 1.3])), 1)
    st = torch.zeros(3, 2)
    b, ctrl = _controller()
    for T in (0, 4097):
        with pytest.raises(ValueError, match=r"n_periods = %d outside \[1, 4096\]" % T):
            b.simulate(st, pd, T)
    with pytest.raises(ValueError, match="warm_up = -1"):
        b.simulate(st, pd, 2, warm_up=-1)
    with pytest.raises(ValueError, match="active has 2 entries"):
        b.simulate(st, pd, 2, active=[1, 0])
    for bad in (torch.ones(3, 3), torch.ones(2, 2), torch.ones(3)):
        with pytest.raises(ValueError, match="plant_params has shape"):
            b.simulate(st, pd, 2, plant_params=bad)
    for kw in (dict(goal=torch.zeros(2)), dict(goal_radius=1.0)):
        with pytest.raises(ValueError, match="come together"):
            b.simulate(st, pd, 2, **kw)
    for goal in (torch.zeros(3), torch.tensor([0.0, float("nan")])):
        with pytest.raises(ValueError, match="goal has shape"):
            b.simulate(st, pd, 2, goal=goal, goal_radius=1.0)
    for r in (0.0, -1.0, float("inf"), float("nan")):
        with pytest.raises(ValueError, match="goal_radius must be finite and > 0"):
            b.simulate(st, pd, 2, goal=torch.zeros(2), goal_radius=r)
    with pytest.raises(ValueError, match="stop_on_crash needs an occupancy map"):
        b.simulate(st, pd, 2, stop_on_crash=True)
    short = SimResult(*(torch.zeros(2) for _ in range(8)))
    with pytest.raises(ValueError, match="resume carries 2 environments"):
        b.simulate(st, pd, 2, resume=short)
    assert b._batch is None and ctrl._ctx is None  # nothing was created: no device call has been made
    p, pctrl = _controller("particle")
    with pytest.raises(ValueError, match="stop_on_crash needs an occupancy map"):
        p.simulate(torch.zeros(3, 4), None, 2, stop_on_crash=True)
    with pytest.raises(ValueError, match="'mass' must be one of the model's uncertain parameters"):
        run_particle_episodes(torch.zeros(3, 4), p.likelihood.model, None, p, load=1.0, steps=8)
    assert p._batch is None and pctrl._ctx is None


# ------------------------------------------------------------------------------------------------ what the GPU test relies on
def test_cases_stay_small():
    for c in cases.CASES:
        assert c["N"] <= 4 and c["S"] <= 16 and c["H"] <= 6 and c["T"] <= 6 and c["B"] <= 5, c["id"]
    assert cases.BY_ID["pend"]["rules"]["warm_up"] == 2 < cases.BY_ID["pend"]["T"]
    one = cases.BY_ID["one"]
    assert (one["N"], one["S"], one["M"], one["H"], one["T"], one["rules"]["warm_up"]) == (1, 1, 1, 1, 1, 1)
    assert any(c["rows"] for c in cases.CASES) and {c["family"] for c in cases.CASES} == {"pendulum", "particle", "skid", "cartpole"}


@pytest.mark.parametrize("cid", sorted(cases.EVENTS))
def test_forced_events_follow_from_the_float64_step(cid):
    """every acceleration of the clamp box crashes environment 0 of `part` in period 0 and keeps environment 1 inside the radius; under
    warm-up the zero action puts both events of `part_warm` into period 1 and not into period 0; the third environment reaches neither
    within T - with at least MARGIN_CELLS / MARGIN_S to spare, so the fp32 predicates of the device decide as float64 does"""
    case = cases.BY_ID[cid]
    got = cases.forced_events(case, cases.grid_of(case))
    print(cid, got)
    assert set(got) == set(range(case["B"]))
    for b, (period, status) in cases.EVENTS[cid].items():
        cells, s = got[b]
        assert (cells if status == 2 else s) >= (cases.MARGIN_CELLS if status == 2 else cases.MARGIN_S)
    assert {st for _, st in cases.EVENTS[cid].values()} == {1, 2} and len(cases.EVENTS[cid]) < case["B"]
    assert {p for p, _ in cases.EVENTS[cid].values()} == ({0} if case["rules"]["warm_up"] == 0 else {1})


@pytest.mark.parametrize("cid", cases.IDS)
def test_cost_tolerance_and_power(cid):
    """From the restatement alone: the cost check's tolerance stays between the floor and the cap, the case shows exactly the variants
    its table row names, and the restated costs lie at least ten times the stated minimum from each of them"""
    case = cases.BY_ID[cid]
    d, tol, power = cases.measure(cid)
    print("%-9s d %.2e tol %.2e  " % (cid, d, tol) + "  ".join("%s %.0f" % kv for kv in sorted(power.items())))
    assert cases.cost_tolerance(case) == tol and cases.TOL_FLOOR <= tol <= cases.TOL_CAP
    assert set(power) == set(cases.COST_POWER[cid]), (sorted(power), sorted(cases.COST_POWER[cid]))
    for v, least in cases.COST_POWER[cid].items():
        assert power[v] >= 10.0 * least, (cid, v, power[v], least)


@pytest.mark.parametrize("cid", ["part", "skid_nav"])
def test_fp32_collision_replica_agrees_with_float64(cid):
    """on points at least MARGIN_CELLS from a cell edge - inside the map, outside it (clamped), far outside - the fp32 replica of the
    device's lookup is amppi_cases._collisions"""
    case = cases.BY_ID[cid]
    grid, cell = cases.grid_of(case), cases.cell_of(case)
    nx, ny = grid.shape
    rng = np.random.default_rng(5)
    idx = rng.integers(-3, max(nx, ny) + 3, (4000, 2)).astype(np.float64)
    frac = rng.uniform(cases.MARGIN_CELLS, 1 - cases.MARGIN_CELLS, (4000, 2))
    edge = rng.random((4000, 2)) < 0.25  # a quarter of the coordinates right at the margin
    frac = np.where(edge, np.where(rng.random((4000, 2)) < 0.5, cases.MARGIN_CELLS, 1 - cases.MARGIN_CELLS), frac)
    xy = ((idx + frac - np.array([int(nx / 2), int(ny / 2)])) * cell)
    xy32 = xy.astype(np.float32)
    want = ac._collisions(grid, xy32.astype(np.float64), cell) != 0
    got = cases.crashed32(grid, xy32, cell)
    assert np.array_equal(got, want) and want.any() and not want.all()
    far = np.array([[1e6, 0.0], [-1e6, 0.0], [0.0, 1e6], [0.0, -1e6]], np.float32)
    assert np.array_equal(cases.crashed32(grid, far, cell), ac._collisions(grid, far.astype(np.float64), cell) != 0)


@pytest.mark.parametrize("cid", ["part", "pend", "skid_nav", "cart"])
def test_fp32_goal_replica_agrees_with_float64(cid):
    """on states whose float64 s lies at least MARGIN_S from r^2 the fp32 expression decides as the float64 norm does"""
    case = cases.BY_ID[cid]
    goal, radius = np.asarray(case["rules"]["goal"], np.float64), case["rules"]["radius"]
    rng = np.random.default_rng(6)
    ds = len(goal)
    dirs = rng.standard_normal((6000, ds))
    dirs /= np.linalg.norm(dirs, axis=1, keepdims=True)
    dist = np.sqrt(rng.uniform(0.0, 2.0 * radius * radius, 6000))
    x32 = (goal + dirs * dist[:, None]).astype(np.float32)
    s = ((goal - x32.astype(np.float64)) ** 2).sum(-1)
    keep = np.abs(s - radius * radius) >= min(cases.MARGIN_S, 0.1 * radius * radius)
    want = np.linalg.norm(goal - x32.astype(np.float64), axis=1) <= radius
    got = cases.goal32(case["rules"]["goal"], radius, x32)
    assert keep.sum() > 5000 and np.array_equal(got[keep], want[keep]) and want[keep].any() and not want[keep].all()
