"""Closed-loop episodes on the device (dust_svmpc_batch_episode, csrc/svmpc_episode.hpp) without a device: the C ABI's new entry and
the Python layers that name it, the register allocation of the five new kernel instances, the refusals of `BatchSVMPC.run_episodes`
that need no device, and the power of the plant check of tests/test_gpu_svmpc_episode.py - its tolerance and its distance from three
wrong plants, from the float64 restatement alone (tests/svmpc_episode_cases.py)."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import __graft_entry__ as entry
import svmpc_episode_cases as cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def built():
    return entry.build()


def test_library_declares_exports_and_binds_the_episode_entry(built):
    from dust_amd import _lib

    lib = C.CDLL(built)
    header = open(os.path.join(ROOT, "include", "dust_amd.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    name = "dust_svmpc_batch_episode"
    assert re.search(r"\b%s\s*\(" % name, code), name + " is not declared"
    assert hasattr(lib, name), name + " is not exported"
    assert name in _lib.SYMBOLS, name + " is not bound"
    assert len(_lib.SYMBOLS[name][1]) == 12
    assert "simulations.py:104-130" in header
    # additive: the version, the ids and the profile counters stay where they were
    assert _lib.load().dust_abi_version() == _lib.ABI_VERSION == 3 and "#define DUST_ABI_VERSION 3" in header
    assert "DUST_K_SVMPC_BATCH = 9" in code and _lib.K_SVMPC_BATCH == 9 and _lib.K_ALL == 10
    assert "DUST_SVB_ACTIONS = 10" in code and "= 11" not in re.search(r"enum dust_svmpc_batch_what \{.*?\}", code, re.S).group(0)


def test_the_python_layers_name_the_episode():
    import dust_amd
    import dust_amd.inference as inf

    assert callable(getattr(dust_amd.SvmpcBatch, "episode", None))
    assert callable(getattr(inf.BatchSVMPC, "run_episodes", None))


def test_episode_kernels_do_not_spill(built, tmp_path):
    """the method of test_svmpc_batch_cpu.py test_batch_kernels_do_not_spill: the gfx950 code object's metadata shows four instances of
    svmpc_episode_kernel and one svmpc_skid_nav_episode_kernel, each without VGPR spill or scratch and within 256 VGPRs"""
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
    plain = {k: v for k, v in kernels.items() if "svmpc_episode_kernel" in k}
    nav = {k: v for k, v in kernels.items() if "svmpc_skid_nav_episode_kernel" in k}
    assert len(plain) == 4 and len(nav) == 1, (sorted(plain), sorted(nav))
    for k, (spill, scratch, vgprs) in list(plain.items()) + list(nav.items()):
        print(k, "spill", spill, "scratch", scratch, "vgprs", vgprs)
        assert spill == 0 and scratch == 0 and vgprs <= 256, (k, spill, scratch, vgprs)  # (512 lanes per workgroup: 256 VGPRs per lane)
    # no new kernel hides in the counts the existing tests take by substring
    for old in ("svmpc_batch_kernel", "svmpc_prior_batch_kernel", "svmpc_skid_nav_batch_kernel", "svmpc_skid_nav_prior_batch_kernel"):
        assert not any(old in k for k in list(plain) + list(nav)), old


def _controller(sampling):
    import torch

    from dust_amd.controllers import MultiDISCO
    from dust_amd.costs import PendulumQuadCos
    from dust_amd.inference import BatchSVMPC, ExponentiatedUtility, get_gmm
    from dust_amd.models import PendulumModel

    N, H, S = 3, 6, 16
    model, cost = PendulumModel(uncertain_params=("length", "mass") if sampling else None), PendulumQuadCos()
    ctrl = MultiDISCO(model.observation_space, model.action_space, H, N, S, a_cov=4.0 * torch.eye(1), inst_cost_fn=cost.inst_cost,
                      term_cost_fn=cost.term_cost, params_sampling=True if sampling else None, params_samples=3)
    prior = get_gmm(torch.zeros(N, H, 1), torch.ones(N), 4.0 * torch.eye(1))
    lik = ExponentiatedUtility(alpha=1.0, n_samples=S, controller=ctrl, model=model)
    return BatchSVMPC(3, torch.zeros(N, H, 1), prior, lik, optimizer_class=torch.optim.SGD, lr=0.5), ctrl


def test_run_episodes_refuses_before_any_device_call():
    import torch
    import torch.distributions as dist

    pd = dist.Independent(dist.Uniform(torch.tensor([0.6, 0.6]), torch.tensor([1.3, 1.3])), 1)
    st = torch.zeros(3, 2)
    b, ctrl = _controller(True)
    for T in (0, 4097):
        with pytest.raises(ValueError, match=r"n_periods = %d outside \[1, 4096\]" % T):
            b.run_episodes(st, pd, T)
    with pytest.raises(ValueError, match="active has 2 entries"):
        b.run_episodes(st, pd, 2, active=[1, 0])
    for bad in (torch.ones(3, 3), torch.ones(2, 2), torch.ones(3)):
        with pytest.raises(ValueError, match="plant_params has shape"):
            b.run_episodes(st, pd, 2, plant_params=bad)
    assert b._batch is None and ctrl._ctx is None  # nothing was created: no device call has been made
    b0, ctrl0 = _controller(False)  # no uncertain parameters: there are no columns a true row could fill
    with pytest.raises(ValueError, match="plant_params has shape"):
        b0.run_episodes(st, None, 2, plant_params=torch.ones(3, 1))
    assert b0._batch is None and ctrl0._ctx is None


def _grid(case):
    if case["family"] == "particle":
        from oracle import grid_4x4_map

        return grid_4x4_map()
    return None


@pytest.mark.parametrize("cid", cases.IDS)
def test_power_of_the_plant_check(cid):
    """From the restatement alone: the tolerance of the plant check stays under the cap, the case shows exactly the variants its table
    row names, and the restated plant lies at least ten times the stated minimum from each of them - so the minimum (POWER) separates a
    wrong plant from rounding with an order of magnitude on both sides."""
    case = cases.BY_ID[cid]
    grid = _grid(case)
    d, tol, power = cases.measure(cid, grid)
    print("%-8s d %.2e tol %.2e  " % (cid, d, tol) + "  ".join("%s %.0f" % kv for kv in sorted(power.items())))
    assert cases.plant_tolerance(case, grid) == tol and cases.TOL_FLOOR <= tol <= cases.TOL_CAP
    assert set(power) == set(cases.POWER[cid]), (sorted(power), sorted(cases.POWER[cid]))
    for v, least in cases.POWER[cid].items():
        assert power[v] >= 10.0 * least, (cid, v, power[v], least)
    # the restated loop against itself passes its own check: the fp32 states it carries are the float64 steps, rounded
    xs, acts, exact = cases.restated_loop(case, grid)
    from helpers import elemerr

    assert elemerr(xs[1:], exact) < tol


def test_the_particle_case_freezes_a_plant():
    """environment 1 of `part` starts on an occupied cell: its positions do not move while its neighbours' do"""
    case = cases.BY_ID["part"]
    xs, _, _ = cases.restated_loop(case, _grid(case))
    assert np.array_equal(xs[1][1, :2], xs[0][1, :2]) and not np.array_equal(xs[1][0, :2], xs[0][0, :2])
