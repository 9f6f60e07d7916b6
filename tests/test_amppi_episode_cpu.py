"""Closed-loop AMPPI episodes on the device (dust_amppi_batch_episode, csrc/amppi_episode.hpp) without a device: the C ABI's new entry
and the Python layers that name it, the register allocation of the seven new kernel instances, the unchanged allocation of the existing
AMPPI instances, the refusals of `BatchAMPPI.run_episodes` that need no device, and the power of the plant check of
tests/test_gpu_amppi_episode.py - its tolerance and its distance from three wrong plants, from the float64 restatement alone
(tests/amppi_episode_cases.py)."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import __graft_entry__ as entry
import amppi_episode_cases as cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (VGPRs, SGPRs, spilled VGPRs, spilled SGPRs, private segment bytes) of every AMPPI kernel the library had before the period kernels
# came, read from a build of the commit before them: amppi_body.inc is included as text, and a new includer must not move them
BEFORE = {
    "_ZN4dust12amppi_kernelILi0EEEvNS_9AmppiArgsE": (57, 106, 0, 2, 0),
    "_ZN4dust12amppi_kernelILi1EEEvNS_9AmppiArgsE": (54, 106, 0, 4, 0),
    "_ZN4dust12amppi_kernelILi2EEEvNS_9AmppiArgsE": (62, 104, 0, 0, 0),
    "_ZN4dust12amppi_kernelILi3EEEvNS_9AmppiArgsE": (69, 106, 0, 3, 0),
    "_ZN4dust17amppi_roll_kernelEPfii": (4, 14, 0, 0, 0),
    "_ZN4dust18amppi_batch_kernelILi0EEEvNS_14AmppiBatchArgsE": (51, 106, 0, 10, 0),
    "_ZN4dust18amppi_batch_kernelILi1EEEvNS_14AmppiBatchArgsE": (47, 106, 0, 12, 0),
    "_ZN4dust18amppi_batch_kernelILi2EEEvNS_14AmppiBatchArgsE": (52, 106, 0, 10, 0),
    "_ZN4dust18amppi_batch_kernelILi3EEEvNS_14AmppiBatchArgsE": (66, 106, 0, 15, 0),
    "_ZN4dust18amppi_prior_kernelILi0EEEvNS_14AmppiPriorArgsE": (42, 48, 0, 0, 0),
    "_ZN4dust18amppi_prior_kernelILi1EEEvNS_14AmppiPriorArgsE": (38, 56, 0, 0, 0),
    "_ZN4dust18amppi_prior_kernelILi2EEEvNS_14AmppiPriorArgsE": (48, 60, 0, 0, 0),
    "_ZN4dust18amppi_prior_kernelILi3EEEvNS_14AmppiPriorArgsE": (54, 54, 0, 0, 0),
    "_ZN4dust21amppi_skid_nav_kernelENS_12AmppiNavArgsE": (63, 106, 0, 3, 0),
    "_ZN4dust23amppi_batch_roll_kernelEPfiiPKh": (4, 14, 0, 0, 0),
    "_ZN4dust24amppi_prior_batch_kernelILi0EEEvNS_19AmppiPriorBatchArgsE": (40, 79, 0, 0, 0),
    "_ZN4dust24amppi_prior_batch_kernelILi1EEEvNS_19AmppiPriorBatchArgsE": (35, 81, 0, 0, 0),
    "_ZN4dust24amppi_prior_batch_kernelILi2EEEvNS_19AmppiPriorBatchArgsE": (42, 83, 0, 0, 0),
    "_ZN4dust24amppi_prior_batch_kernelILi3EEEvNS_19AmppiPriorBatchArgsE": (52, 82, 0, 0, 0),
    "_ZN4dust27amppi_skid_nav_batch_kernelENS_17AmppiNavBatchArgsE": (55, 106, 0, 18, 0),
    "_ZN4dust27amppi_skid_nav_prior_kernelENS_17AmppiNavPriorArgsE": (48, 71, 0, 0, 0),
    "_ZN4dust33amppi_skid_nav_prior_batch_kernelENS_22AmppiNavPriorBatchArgsE": (46, 92, 0, 0, 0),
}


@pytest.fixture(scope="module")
def built():
    return entry.build()


@pytest.fixture(scope="module")
def kernels(built, tmp_path_factory):
    """name -> (VGPRs, SGPRs, spilled VGPRs, spilled SGPRs, private segment bytes) from the gfx950 code object's metadata"""
    llvm = "/opt/rocm/lib/llvm/bin"
    if not (os.path.exists(llvm + "/llvm-objdump") and os.path.exists(llvm + "/llvm-readelf")):
        pytest.skip("llvm-objdump / llvm-readelf not available")
    tmp = str(tmp_path_factory.mktemp("co"))
    shutil.copy(built, os.path.join(tmp, "l.so"))
    subprocess.run([llvm + "/llvm-objdump", "--offloading", "l.so"], cwd=tmp, check=True, capture_output=True)
    co = [f for f in os.listdir(tmp) if "gfx950" in f]
    assert co, "no gfx950 code object in libdust_amd.so"
    notes = "".join(subprocess.run([llvm + "/llvm-readelf", "--notes", f], cwd=tmp, check=True, capture_output=True, text=True).stdout for f in co)
    out = {}
    for m in re.finditer(r"\.name:\s+(\S+)\n(.*?)\.wavefront_size", notes, re.S):
        g = lambda k: int(re.search(r"\.%s:\s+(\d+)" % k, m.group(2)).group(1))
        out[m.group(1)] = (g("vgpr_count"), g("sgpr_count"), g("vgpr_spill_count"), g("sgpr_spill_count"), g("private_segment_fixed_size"))
    return out


def test_library_declares_exports_and_binds_the_episode_entry(built):
    from dust_amd import _lib

    lib = C.CDLL(built)
    header = open(os.path.join(ROOT, "include", "dust_amd.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    name = "dust_amppi_batch_episode"
    assert re.search(r"\b%s\s*\(" % name, code), name + " is not declared"
    assert hasattr(lib, name), name + " is not exported"
    assert name in _lib.SYMBOLS, name + " is not bound"
    FP, UB = _lib.FP, C.POINTER(C.c_ubyte)
    assert _lib.SYMBOLS[name] == (C.c_int, [_lib.VP, FP, C.c_int, FP, C.c_int, C.c_int, FP, UB, FP, FP, FP, FP, FP])
    dual = "dust_amppi_dual_batch_episode"
    assert re.search(r"\b%s\s*\(" % dual, code) and hasattr(lib, dual) and dual in _lib.SYMBOLS, dual
    assert _lib.SYMBOLS[dual] == (C.c_int, [_lib.VP, _lib.VP, FP, FP, C.c_int, C.c_int, C.c_int, C.c_float, C.POINTER(C.c_uint64), C.c_int, FP, UB,
                                            FP, FP, FP, FP, FP, FP])
    # additive: the version and the profile counters stay where they were
    assert _lib.load().dust_abi_version() == _lib.ABI_VERSION == 3 and "#define DUST_ABI_VERSION 3" in header
    assert _lib.K_ALL == 10


def test_the_python_layers_name_the_episode():
    import dust_amd
    from dust_amd.controllers import BatchAMPPI

    from dust_amd.controllers import BatchDualAMPPI

    assert callable(getattr(dust_amd.AmppiBatch, "episode", None)) and callable(getattr(dust_amd.AmppiBatch, "dual_episode", None))
    assert callable(getattr(BatchAMPPI, "run_episodes", None)) and callable(getattr(BatchDualAMPPI, "run_episodes", None))


def test_period_kernels_do_not_spill(kernels):
    """four instances of amppi_period_kernel, one amppi_skid_nav_period_kernel and the Pendulum and Particle instances of
    amppi_prior_period_kernel, each without VGPR spill or scratch, within 256 VGPRs"""
    plain = {k: v for k, v in kernels.items() if "amppi_period_kernel" in k}
    nav = {k: v for k, v in kernels.items() if "amppi_skid_nav_period_kernel" in k or "amppi_prior_period_kernel" in k}
    assert len(plain) == 4 and len(nav) == 3, (sorted(plain), sorted(nav))
    for k, (vgprs, sgprs, spill, sspill, scratch) in list(plain.items()) + list(nav.items()):
        print(k, "vgprs", vgprs, "sgprs", sgprs, "spill", spill, "scratch", scratch)
        assert spill == 0 and scratch == 0 and vgprs <= 256, (k, spill, scratch, vgprs)
    # no new kernel hides in the counts the existing tests take by substring
    for old in ("amppi_kernel", "amppi_batch_kernel", "amppi_skid_nav_batch_kernel", "amppi_prior_kernel", "amppi_skid_nav_prior_kernel"):
        assert not any(old in k for k in list(plain) + list(nav)), old


def test_existing_amppi_kernels_keep_their_registers(kernels):
    """every AMPPI kernel from before the period kernels is still there with the register figures it had, and the period kernels are the
    only AMPPI kernels that came"""
    mine = {k: v for k, v in kernels.items() if "amppi" in k and "period" not in k}
    assert set(mine) == set(BEFORE), sorted(set(mine) ^ set(BEFORE))
    for k, want in BEFORE.items():
        assert mine[k] == want, (k, mine[k], want)


def _pend(up=("length",)):
    from dust_amd.costs import PendulumQuadCos
    from dust_amd.models import PendulumModel

    return PendulumModel(uncertain_params=up), PendulumQuadCos()


def test_run_episodes_refuses_before_any_device_call():
    import torch

    from dust_amd.controllers import BatchAMPPI

    m, c = _pend()
    kw = dict(inst_cost_fn=c.inst_cost, term_cost_fn=c.term_cost)
    b = BatchAMPPI(3, m.observation_space, m.action_space, 8, 64, **kw)
    st = torch.zeros(3, 2)
    for T in (0, 4097):
        with pytest.raises(ValueError, match=r"n_periods = %d outside \[1, 4096\]" % T):
            b.run_episodes(m, st, T)
    with pytest.raises(ValueError, match="steps >= 1"):
        b.run_episodes(m, st, 2, roll_steps=0)
    with pytest.raises(ValueError, match="active has 2 entries"):
        b.run_episodes(m, st, 2, active=[1, 0])
    for bad in (torch.ones(3, 2), torch.ones(2, 1), torch.ones(3)):
        with pytest.raises(ValueError, match="plant_params has shape"):
            b.run_episodes(m, st, 2, plant_params=bad)
    assert b._batch is None  # nothing was created: no device call has been made
    m0, _ = _pend(None)  # no uncertain parameters: there are no columns a true row could fill
    b0 = BatchAMPPI(3, m0.observation_space, m0.action_space, 8, 64, params_sampling="none", **kw)
    with pytest.raises(ValueError, match="plant_params has shape"):
        b0.run_episodes(m0, st, 2, plant_params=torch.ones(3, 1))
    assert b0._batch is None


def _grid(case):
    if case["family"] == "particle":
        from oracle import grid_4x4_map

        return grid_4x4_map()
    return None


@pytest.mark.parametrize("cid", cases.IDS + [cases.DUAL_PLANT["id"]])
def test_power_of_the_plant_check(cid):
    """From the restatement alone: the tolerance of the plant check stays between floor and cap, the case shows exactly the variants
    its row can show, and the restated plant lies RESTATED_MARGIN times the demanded POWER from each of them in at least one period"""
    case = cases.BY_ID[cid]
    grid = _grid(case)
    d, tol, power = cases.measure(cid, grid)
    print("%-10s d %.2e tol %.2e  " % (cid, d, tol) + "  ".join("%s %.0f" % kv for kv in sorted(power.items())))
    assert cases.plant_tolerance(case, grid) == tol and cases.TOL_FLOOR <= tol <= cases.TOL_CAP
    assert set(power) == cases.variants_of(case), (sorted(power), sorted(cases.variants_of(case)))
    for v, got in power.items():
        assert got >= cases.RESTATED_MARGIN * cases.POWER, (cid, v, got)
    # the restated loop against itself passes its own check: the fp32 states it carries are the float64 steps, rounded
    xs, acts, exact = cases.restated_loop(case, grid)
    from helpers import elemerr

    assert elemerr(xs[1:], exact) < tol


def test_the_table_covers_what_it_names():
    """the sizes at which the kernel takes another path, and the true rows 10 - 40 % off the nominal ones"""
    by = cases.BY_ID
    assert {by[k]["S"] for k in ("s1", "s255", "s256_d30", "s257_edge", "s1021_ut")} == {1, 255, 256, 257, 1021}
    D = {k: c["H"] * cases.family(c)["da"] for k, c in by.items()}
    assert D["d1"] == 1 and D["s256_d30"] == 30 and D["d128"] == 128 and by["d1"]["roll_steps"] == 1 and by["skid_cov"]["roll_steps"] == 3
    assert {c["family"] for c in cases.CASES} == {"pendulum", "particle", "skid", "cartpole"}
    assert {c["mode"] for c in cases.CASES} == {"none", "single", "extended", "ut"}
    assert by["nav_lds"]["nav"] and by["nav_dev"]["nav"] and by["nav_dev"]["map_dev"] and not by["nav_lds"]["map_dev"]
    for c in cases.CASES:
        if c["true_rel"] is not None:
            rel = np.abs(np.asarray(c["true_rel"]) - 1.0)
            assert (rel >= 0.1 - 1e-12).all() and (rel <= 0.4 + 1e-12).all(), c["id"]
        assert c["T"] <= 4 and c["B"] <= 5


def test_the_particle_case_freezes_a_plant():
    """environment 1 of `part` starts on an occupied cell: its positions do not move while its neighbours' do"""
    case = cases.BY_ID["part"]
    xs, _, _ = cases.restated_loop(case, _grid(case))
    assert np.array_equal(xs[1][1, :2], xs[0][1, :2]) and not np.array_equal(xs[1][0, :2], xs[0][0, :2])


def test_dual_run_episodes_key_schedule_and_refusals_before_any_device_call():
    """period t of a piece that starts after _t periods draws under prior_keys(_t + 1 + t) = seed + (b << 32) + _t + 1 + t, the schedule
    `BatchDualSVMPC.run_episodes` documents; n_periods, the roll, a skid-steer pair and the plant rows are refused on the host"""
    import torch

    from dust_amd.controllers import BatchAMPPI, BatchDualAMPPI

    m, c = _pend(("length", "mass"))
    ctrl = BatchAMPPI(3, m.observation_space, m.action_space, 8, 64, inst_cost_fn=c.inst_cost, term_cost_fn=c.term_cost)
    seen = {}

    class Batch:  # stands in for the device batch: records what run_episodes hands down
        da = 1

        def dual_episode(self, mb, st, T, ap, **kw):
            seen.update(kw, T=T, ap=ap)
            z = lambda *sh: np.zeros(sh, np.float32)
            return z(T, 3, 2), z(T, 3, 1), z(T, 3, 64), z(T, 3, 64), z(T, 3), z(3, 8, 1)

    class Filters:
        class _dev:
            P = 2

        class likelihood:
            log_space = False
            model = None

        prior = None

    dual = BatchDualAMPPI.__new__(BatchDualAMPPI)
    dual.controller, dual.model, dual.mpf, dual.roll = ctrl, m, Filters, 1
    dual.n_envs, dual._seed, dual._t, dual._pending, dual.mpf_steps, dual.mpf_bw, dual.ticks, dual.last_bw = 3, 1000, 4, None, 5, None, 4, None
    st = torch.zeros(3, 2)
    for T in (0, 4097):
        with pytest.raises(ValueError, match=r"n_periods = %d outside \[1, 4096\]" % T):
            dual.run_episodes(st, T)
    with pytest.raises(ValueError, match="plant_params has shape"):
        dual.run_episodes(st, 2, plant_params=torch.ones(3, 1))
    with pytest.raises(ValueError, match="active has 2 entries"):
        dual.run_episodes(st, 2, active=[1, 0])
    dual.roll = 0
    with pytest.raises(ValueError, match="roll >= 1"):
        dual.run_episodes(st, 2)
    dual.roll = 1
    assert ctrl._batch is None and seen == {}  # nothing was created: no device call has been made
    ctrl._ensure_batch = lambda model: Batch()
    dual._filters = lambda states: None
    dual.run_episodes(st, 3, active=[1, 0, 1])
    want = [[1000 + (b << 32) + 4 + 1 + t for b in range(3)] for t in range(3)]
    assert np.array_equal(seen["seeds"], np.array(want, np.uint64)) and seen["T"] == 3 and seen["ap"] is None and seen["roll_steps"] == 1
    assert dual._t == 7 and dual.ticks == 7 and dual._pending[0].shape == (3, 1) and dual._pending[1].shape == (3, 2)
    assert [dual.prior_keys(5)[b] for b in range(3)] == want[0]
