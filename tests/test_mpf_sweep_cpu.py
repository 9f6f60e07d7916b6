"""Per-environment filter hyper-parameters (dust_mpf_batch_set_hyper / _get_hyper; csrc/mpf.hpp mpf_optimize_rows_kernel,
mpf_silverman_rows_kernel) without a device: the C ABI's two entries and their struct, the register allocation of the new kernel
instances beside the unchanged figures of the existing ones, the Python refusals that need no device, and the case table of
tests/mpf_sweep_cases.py."""
import ctypes as C
import inspect
import math
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import __graft_entry__ as entry
import mpf_sweep_cases as sw
from test_svmpc_dual_episode_cpu import _NoDevice, _dual

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# What the parent commit's build shows (tools/kernel_regs.py), and this change must not move: the sorted VGPR counts of the 44 instances
# of mpf_optimize_batch_kernel, (spilled VGPRs, scratch bytes, VGPRs) of mpf_silverman_batch_kernel, and (spilled VGPRs, scratch bytes)
# of the lone kernel's eight instances by (P, CART)
MPF_VGPRS = [77, 77, 80, 80, 83, 84, 84, 87, 87, 87, 93, 95, 95, 95, 96, 98, 99, 99, 102, 103, 105, 109, 109, 110, 110, 111, 111, 114, 116, 118, 119,
             119, 120, 121, 121, 121, 121, 122, 124, 125, 125, 125, 125, 128]
LONE = {(1, 1): (0, 0), (1, 0): (4, 20), (2, 1): (0, 0), (2, 0): (20, 84), (3, 1): (0, 0), (3, 0): (38, 156), (4, 1): (7, 32), (4, 0): (45, 184)}


@pytest.fixture(scope="module")
def built():
    return entry.build()


def _kernels(built, tmp_path):
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
    return kernels


def test_library_declares_exports_and_binds_the_entries(built):
    from dust_amd import _lib

    lib = C.CDLL(built)
    header = open(os.path.join(ROOT, "include", "dust_amd.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    want = {"dust_mpf_batch_set_hyper": ["dust_mpf_batch *batch", "const dust_mpf_hyper *rows"],
            "dust_mpf_batch_get_hyper": ["dust_mpf_batch *batch", "dust_mpf_hyper *rows"]}
    for name, args in want.items():
        decl = re.search(r"\bint\s+%s\s*\((.*?)\)\s*;" % name, code, re.S)
        assert decl, name + " is not declared"
        assert [" ".join(a.split()) for a in decl.group(1).split(",")] == args, name
        assert hasattr(lib, name), name + " is not exported"
        assert _lib.SYMBOLS.get(name) == (C.c_int, [_lib.VP, C.POINTER(_lib.MpfHyper)]), name
    # additive: the version stays
    assert _lib.load().dust_abi_version() == _lib.ABI_VERSION and "#define DUST_ABI_VERSION %d" % _lib.ABI_VERSION in header


def test_the_struct_layout_comes_from_a_c_compile(tmp_path):
    """dust_mpf_hyper's size and offsets as a C compiler lays the header's struct out, against the ctypes mirror"""
    from dust_amd import _lib

    cc = shutil.which("cc") or shutil.which("gcc")
    if cc is None:
        pytest.skip("no C compiler")
    src = tmp_path / "layout.c"
    fields = ("lr", "obs_std", "bw", "bw_scale", "reserved")
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "dust_amd.h"\nint main(void) {\n  printf("%zu", sizeof(dust_mpf_hyper));\n'
                   + "".join('  printf(" %%zu", offsetof(dust_mpf_hyper, %s));\n' % f for f in fields) + '  printf("\\n");\n  return 0;\n}\n')
    exe = str(tmp_path / "layout")
    subprocess.run([cc, "-I" + os.path.join(ROOT, "include"), str(src), "-o", exe], check=True, capture_output=True)
    got = [int(v) for v in subprocess.run([exe], check=True, capture_output=True, text=True).stdout.split()]
    assert got == [24, 0, 8, 12, 16, 20], got
    assert C.sizeof(_lib.MpfHyper) == got[0]
    assert [getattr(_lib.MpfHyper, f).offset for f in fields] == got[1:]
    assert _lib.MpfHyper.lr.size == 8 and all(getattr(_lib.MpfHyper, f).size == 4 for f in fields[1:])


def test_the_rows_kernels_do_not_spill_and_the_existing_ones_keep_their_registers(built, tmp_path):
    """exactly 16 instances of mpf_optimize_rows_kernel<P, MODEL, LOG, ADAM> - Pendulum P = 1 .. 3 and Particle P = 1, x parameter space x
    (Adam, any other optimiser) - and one mpf_silverman_rows_kernel, each without VGPR spill or scratch and within the 128 VGPRs of a
    1 024-lane workgroup: the figures the 44 uniform instances have.  Those, the uniform Silverman kernel and the lone kernel's eight
    instances show the parent's figures."""
    kernels = _kernels(built, tmp_path)
    new = {k: v for k, v in kernels.items() if "mpf_optimize_rows_kernel" in k}
    assert len(new) == 16, sorted(new)
    want = {"_ZN4dust24mpf_optimize_rows_kernelILi%dELi%dELb%dELb%dEEEvNS_11MpfRowsArgsE" % (P, model, lg, adam)
            for model, Ps in ((0, (1, 2, 3)), (1, (1,))) for P in Ps for lg in (0, 1) for adam in (0, 1)}
    assert set(new) == want, sorted(set(new) ^ want)
    silver = {k: v for k, v in kernels.items() if "mpf_silverman_rows_kernel" in k}
    assert len(silver) == 1, sorted(silver)
    for k, (spill, scratch, vgprs) in list(new.items()) + list(silver.items()):
        print(k, "spill", spill, "scratch", scratch, "vgprs", vgprs)
        assert spill == 0 and scratch == 0 and vgprs <= 128, (k, spill, scratch, vgprs)
    for old in ("mpf_optimize_batch_kernel", "mpf_silverman_batch_kernel", "mpf_optimize_kernel"):
        assert not any(old in k for k in list(new) + list(silver)), old  # no new kernel hides in the counts existing tests take by substring
    old = {k: v for k, v in kernels.items() if "mpf_optimize_batch_kernel" in k}
    assert len(old) == 44 and all(v[0] == 0 and v[1] == 0 for v in old.values()), sorted(old)
    assert sorted(v[2] for v in old.values()) == MPF_VGPRS
    uni = [v for k, v in kernels.items() if "mpf_silverman_batch_kernel" in k]
    assert len(uni) == 1 and uni[0][:2] == (0, 0), uni
    for (P, cart), (spill, scratch) in LONE.items():
        name = "_ZN4dust19mpf_optimize_kernelILi%dELb%dEEEvNS_7MpfArgsE" % (P, cart)
        assert kernels[name][:2] == (spill, scratch), (name, kernels[name])


def test_the_python_layers_name_the_entries():
    import dust_amd
    import dust_amd.controllers as ctl
    from dust_amd.utils import simulations

    assert callable(getattr(dust_amd.MpfBatch, "set_hyper", None)) and isinstance(dust_amd.MpfBatch.hyper, property)
    assert dust_amd.MpfBatch.HYPER_FIELDS == sw.FIELDS
    for cls in (ctl.BatchDualSVMPC, ctl.BatchDualAMPPI):
        assert callable(getattr(cls, "set_filter_hyper", None)) and isinstance(cls.filter_hyper, property), cls
    assert inspect.signature(simulations.run_pendulum_simulations).parameters["mpf_hyper"].default is None
    assert inspect.signature(simulations.run_particle_episodes).parameters["mpf_hyper"].default is None


def test_the_python_refusals_come_ahead_of_any_device_call():
    import torch

    from dust_amd import MpfBatch
    from dust_amd.models import PendulumModel
    from dust_amd.utils.simulations import run_particle_episodes

    rows = [dict(lr=1e-3), dict(bw=0.05), dict(obs_std=0.1)]
    d, sv, ctrl = _dual(PendulumModel(uncertain_params=("length", "mass")))
    d.mpf_bw = 0.05  # (what the constructor was given)
    with pytest.raises(ValueError, match="put it in the rows"):
        d.set_filter_hyper(rows)
    d.set_filter_hyper(None)  # (clearing needs no bandwidth)
    d.mpf_bw = None
    with pytest.raises(ValueError, match="2 rows for 3 environments"):
        d.set_filter_hyper(rows[:2])
    d.set_filter_hyper(rows)  # kept for the filters the first forward() makes
    assert d._filter_hyper == rows and d._filter_hyper is not rows
    assert sv._batch is None and ctrl._ctx is None and d._mb is None  # nothing was created: no device call has been made
    # the binding checks the rows' shape and names ahead of the library
    b = MpfBatch.__new__(MpfBatch)
    b._h, b.B, b._proto_hyper = _NoDevice(), 3, dict(lr=1e-3, obs_std=0.1, bw=0.0, bw_scale=1.0)
    for bad in (rows[:2], [dict(r, alpha=1.0) for r in rows], np.zeros(3, [("lr", np.float64), ("sigma", np.float32)])):
        with pytest.raises(ValueError):
            b.set_hyper(bad)
    b._h = None  # (nothing to destroy)
    with pytest.raises(ValueError, match="pass the filter prototype as mpf"):
        run_particle_episodes(torch.zeros(3, 4), None, None, sv, mpf=None, mpf_hyper=rows)


def test_case_table_rows_are_valid_and_pairwise_distinct():
    assert sw.B == 5 and set(sw.SIZES) >= {1, 3, 65, 130}
    assert {len(sw.CASES[c]["up"]) for c, _ in sw.GRID} == {1, 2, 3} and {Mp for _, Mp in sw.GRID} == set(sw.SIZES)
    assert any(c["opt"] == "Adam" and c["log"] for c in sw.CASES.values()) and any(c["family"] == "particle" and c["log"] for c in sw.CASES.values())
    for case in sw.CASES:
        rows, p = sw.rows(case), sw.proto_row(case)
        assert len(rows) == sw.B and rows[0] == p
        for r in rows:
            assert sorted(r) == sorted(sw.FIELDS)
            assert all(math.isfinite(r[k]) for k in sw.FIELDS) and r["lr"] > 0 and r["obs_std"] > 0 and r["bw_scale"] > 0
            assert all(r[k] == float(np.float32(r[k])) for k in sw.FIELDS)  # (a filter created with the row holds the same bits)
        keys = [tuple(r[k] for k in sw.FIELDS) for r in rows]
        assert len(set(keys)) == sw.B
        assert rows[1]["lr"] == 4 * p["lr"] and rows[2]["obs_std"] == sw.f32(0.5 * p["obs_std"]) and rows[3]["bw_scale"] == 0.5
        assert rows[4]["bw"] == sw.f32(0.05) and sum(r["bw"] > 0 for r in rows) == 1
        for f in sw.FIELDS:
            v = sw.other_value(case, f)
            assert v != p[f] and math.isfinite(v) and v > 0
    for field, value in sw.INVALID:  # each is invalid by the header's rule, and every field that can be is covered
        assert not math.isfinite(value) or (field != "bw" and value <= 0)
    assert {f for f, _ in sw.INVALID} == set(sw.FIELDS)
