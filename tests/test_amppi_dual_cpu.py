"""The AMPPI dual loop without a device: the C ABI's new entry, the register allocation of the tick's new kernel instances (the ones that
draw their parameter row themselves), DualAMPPI's constructor refusals, and the fixtures of the reference's composed loop
(tests/golden/amppi_dual_*.npz): stored conditions, float64 restatements, the generator's dry run."""
import ctypes as C
import os
import re
import subprocess
import sys
import types

import pytest

import __graft_entry__ as entry

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _dual():
    import amppi_dual_cases as dc

    return dc


@pytest.fixture(scope="module")
def built():
    return entry.build()


def test_library_exports_and_binds_the_dual_tick(built):
    from dust_amd import _lib

    lib = C.CDLL(built)
    assert hasattr(lib, "dust_amppi_dual_tick") and "dust_amppi_dual_tick" in _lib.SYMBOLS
    assert len(_lib.SYMBOLS["dust_amppi_dual_tick"][1]) == 15
    assert _lib.load().dust_abi_version() == _lib.ABI_VERSION == 3
    header = open(os.path.join(ROOT, "include", "dust_amd.h")).read()
    assert "#define DUST_ABI_VERSION 3" in header
    decl = re.search(r"int dust_amppi_dual_tick\((.*?)\);", header, re.S)
    assert decl and len(decl.group(1).split(",")) == 15
    from dust_amd import Context
    from dust_amd.controllers import DualAMPPI  # noqa: F401

    assert callable(Context.amppi_dual_tick)


def test_prior_kernels_do_not_spill(built, tmp_path):
    """the method of test_amppi_kernels_do_not_spill: the gfx950 code object's metadata shows no VGPR spill and no scratch for the five
    instances that draw their parameter row in registers (the four families and skid-steer with the navigation cost) - a row read as
    row[col] under a run-time column would live in scratch memory"""
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
    mine = {k: v for k, v in kernels.items() if "amppi_prior_kernel" in k or "amppi_skid_nav_prior_kernel" in k}
    assert len(mine) == 5, sorted(mine)
    for k, (spill, scratch, vgprs) in mine.items():
        assert spill == 0 and scratch == 0 and vgprs <= 128, (k, spill, scratch, vgprs)


def _stub_mpf(log_space):
    return types.SimpleNamespace(likelihood=types.SimpleNamespace(log_space=log_space), draw_source=None)


def _controller(sampling):
    from dust_amd.controllers import AMPPI
    from dust_amd.costs import PendulumQuadCos
    from dust_amd.models import PendulumModel

    model, pc = PendulumModel(uncertain_params=("length",)), PendulumQuadCos()
    return AMPPI(model.observation_space, model.action_space, 8, 64, inst_cost_fn=pc.inst_cost, term_cost_fn=pc.term_cost, params_sampling=sampling), model


def test_constructor_refusals_need_no_device():
    from dust_amd.controllers import DualAMPPI

    ctrl, model = _controller("extended")
    with pytest.raises(NotImplementedError, match="log-space"):
        DualAMPPI(ctrl, model, _stub_mpf(True))
    none, model = _controller("none")
    with pytest.raises(ValueError, match="none"):
        DualAMPPI(none, model, _stub_mpf(False))
    with pytest.raises(ValueError, match="roll"):
        DualAMPPI(ctrl, model, _stub_mpf(False), roll=-1)
    assert none._ctx is None and ctrl._ctx is None  # no device call was made
    loop = DualAMPPI(ctrl, model, _stub_mpf(False), mpf_bw=0.1, mpf_steps=5, fused=True, seed=3, roll=2)
    assert (loop.mpf_bw, loop.mpf_steps, loop.fused, loop.roll, loop.last_bw, loop.ticks) == (0.1, 5, True, 2, None, 0)


def test_fused_falls_back_for_a_custom_root_or_another_parameter_count():
    from dust_amd.controllers import DualAMPPI
    from dust_amd.utils.utf import MerweScaledUTF

    def fuses(tf, P):
        ctrl, model = _controller(tf)
        mpf = _stub_mpf(False)
        mpf._dev = types.SimpleNamespace(P=P)
        return DualAMPPI(ctrl, model, mpf, fused=True)._can_fuse()

    assert fuses(MerweScaledUTF(n=1, alpha=1.0), 1)
    assert not fuses(MerweScaledUTF(n=1, alpha=1.0), 2)
    assert not fuses(MerweScaledUTF(n=1, alpha=1.0, sqrt_method=lambda a: a), 1)
    assert fuses("extended", 1) and fuses("single", 1)


# ---------------------------------------------------------------------------------------------- the fixtures
@pytest.mark.parametrize("name", _dual().NAMES)
def test_fixture_conditions(golden, name):
    """per-period tolerances = max(1e-5, 2 d) under the cap; top weight <= 0.5; the update moves a_seq and every filter update moves the
    particles by >= 100 tolerances; each power variant >= 10 tolerances from the truth; the inputs are the cases file's"""
    import numpy as np
    from helpers import elemerr

    dc = _dual()
    s, g = dc.BY_TAG[name], golden("amppi_dual_" + name)
    T = int(g["T"])
    assert T == dc.TICKS
    for q in dc.QUANT + ("plant",):
        tol = np.asarray(g["tol_" + q])
        assert tol.shape == (T,) and (tol >= dc.TOL).all() and (tol <= dc.CAP).all(), q
        for k in range(T):
            assert elemerr(g[q][k], g[q + "_f64"][k]) <= tol[k] / 2 * (1 + 1e-6), (q, k)
    assert float(np.exp(g["omega"]).max()) <= 0.5
    inp = dc.inputs(s)
    for k in ("state", "a_seq0", "x0"):
        assert np.array_equal(g[k], inp[k]), k
    prev_x, prev_a = g["x0"], g["a_seq0"]
    for k in range(T):
        assert elemerr(g["a_seq1"][k], prev_a) >= 100 * float(g["tol_a_seq1"][k]), k
        assert elemerr(g["x"][k], prev_x) >= 100 * float(g["tol_x"][k]), k
        prev_x, prev_a = g["x"][k], np.concatenate([g["a_seq1"][k][1:], np.zeros_like(g["a_seq0"][:1])])
    assert {v[6:] for v in g if v.startswith("costs_") and v != "costs_f64"} == set(dc.variants_of(s))
    for v in dc.variants_of(s):
        for k in range(1 if v == "stale" else 0, T):
            assert elemerr(g["costs_" + v][k], g["costs"][k]) >= 10 * float(g["tol_costs"][k]), (v, k)
    assert (g["bw_in"] < 0) == (s["bw"] is None)


@pytest.mark.parametrize("name", _dual().NAMES)
def test_controller_half_restated_is_the_float64_twin(golden, name):
    """every period's update restated in float64 numpy (amppi_cases.restate on the reference's own sequence, plant state and recorded
    rows) reproduces the float64 run to 1e-12, and its variants are the stored power variants"""
    import numpy as np
    from helpers import elemerr

    dc = _dual()
    s, g = dc.BY_TAG[name], golden("amppi_dual_" + name)
    for k in range(int(g["T"])):
        r = dc.restate_costs(s, g, k, None)
        for q in ("costs", "omega", "a_seq1"):
            assert elemerr(r[q], g[q + "_f64"][k]) < 1e-12, (q, k)
        for v in dc.variants_of(s):
            if v == "stale" and k == 0:
                continue
            assert np.array_equal(dc.restate_costs(s, g, k, v)["costs"].astype(np.float32), g["costs_" + v][k]), (v, k)


def test_dual_fixture_files_are_small():
    for n in _dual().NAMES:
        assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "amppi_dual_" + n + ".npz")) < 512 * 1024, n


@pytest.mark.parametrize("name", _dual().NAMES)
def test_plant_and_bandwidth_restated_are_the_float64_twins(golden, name, built):
    """the rest of a period that numpy restates: the plant's step under the first row of the updated sequence, and the bandwidth of the
    filter update - Silverman's rule of the particles the update started from (mpf.py:68-73) where the fixture has bw = None.  (The
    filter's SVGD steps themselves, x_f64, are not restated here: the MPF fixtures hold them.)"""
    import numpy as np
    from helpers import elemerr

    dc = _dual()
    s, g = dc.BY_TAG[name], golden("amppi_dual_" + name)
    for k in range(int(g["T"])):
        assert elemerr(dc.restate_plant(s, g, k), g["plant_f64"][k]) < 1e-12, k
        want = float(np.asarray(g["bw_f64"][k]).reshape(-1)[0])
        assert abs(dc.restate_bw(s, g, k) - want) <= 1e-12 * abs(want), k


def test_generator_dry_table_reproduces_the_stored_tolerances(golden):
    """when the reference tree is present: the committed generator, run dry, gives the stored fixtures again"""
    import json

    import numpy as np
    from oracle import ref_shim

    if not os.path.isdir(os.path.join(ref_shim.REFERENCE_ROOT, "dust")):
        pytest.skip("the reference tree is not on this machine")
    tags = list(_dual().NAMES)
    code = ("import sys, json, numpy as np; sys.argv = ['x']; sys.path.insert(0, %r); import make_golden_amppi_dual as G; out = {}\n"
            "for t in %r:\n"
            "    g = G.run(G.cases.BY_TAG[t], write=False)\n"
            "    out[t] = {k: np.asarray(v, np.float64).reshape(-1).tolist() for k, v in g.items() if k.startswith('tol_')}\n"
            "    for q in ('costs', 'x', 'bw'):\n"
            "        out[t][q] = np.asarray(g[q], np.float64).reshape(-1)[:8].tolist()\n"
            "print('TABLE' + json.dumps(out))\n") % (os.path.join(ROOT, "tests", "golden"), tags)
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True, check=True)
    table = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("TABLE")][0][5:])
    for t in tags:
        g = golden("amppi_dual_" + t)
        assert set(k for k in g if k.startswith("tol_")) == set(k for k in table[t] if k.startswith("tol_")), t
        for k, v in table[t].items():
            want = np.asarray(g[k], np.float64).reshape(-1)
            assert np.array_equal(np.asarray(v), want if k.startswith("tol_") else want[:8]), (t, k)
