"""The sigma-point mode of the skid-steer and cart-pole families without a GPU: the fixtures of tests/golden/make_golden_ut_families.py keep
their caps and their power, a float64 numpy restatement of the weighted cost (ut_cases.ut_costs) reproduces the reference's float64
costs from its float64 states, the library exports and declares the two new entries, the three kernels compile without spills or
scratch, and the host MerweScaledUTF gives the reference's sigma points and weights."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

import __graft_entry__ as entry
from cartpole_cases import TICK_QUANT
from helpers import elemerr
from ut_cases import (CAP, FAMILY, ROLLOUT_BY_TAG, ROLLOUT_NAMES, ROLLOUT_QUANT, SIGMA_BY_TAG, SIGMA_NAMES, SIGMA_SIZES, TICK_BY_TAG, TICK_NAMES, TOL,
                      dist_of, sigma_particles, twin, ut_costs, weights)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def built():
    return entry.build()


def _check_quantity(g, q, per_slice=False):
    tol = float(g["tol_" + q])
    assert TOL <= tol <= CAP, (q, tol)
    t64 = twin(g, q)
    d = max(elemerr(a, b) for a, b in zip(g[q], t64)) if per_slice else elemerr(g[q], t64)
    assert 2.0 * d <= tol * (1 + 1e-12) + (0.0 if q + "_f64" in g else 1e-12), (q, d, tol)


# ---------------------------------------------------------------------------------------------- the fixtures
@pytest.mark.parametrize("name", ROLLOUT_NAMES)
def test_rollout_fixture_caps_power_and_closed_form(golden, name):
    g, s = golden("ut_" + name), ROLLOUT_BY_TAG[name]
    f = FAMILY[s["family"]]
    P, pts = len(s["up"]), 2 * len(s["up"]) + 1
    for q in ROLLOUT_QUANT:
        if q != "states" or s["states"]:
            _check_quantity(g, q)
    assert elemerr(g["costs_off"], g["costs"]) >= 10 * float(g["tol_costs"])
    assert s["N"] * s["S"] == 300 and s["H"] == 7  # one full 256-lane block and a ragged one; H coprime with 3, 5, 9 (= 7 points at P = 3)
    assert g["costs"].shape == (s["S"], s["N"]) and g["sigma_points"].shape == (pts, P) and int(g["M"]) == pts
    w, scale = weights(P, float(g["alpha"]))
    assert np.allclose(g["loc_weights"], w, rtol=1e-6) and abs(float(g["sigma_scale"]) - scale) < 1e-12 and abs(w.sum() - 1.0) < 1e-12
    mean, std = dist_of(s)
    assert np.array_equal(g["dist_mean"], mean) and np.array_equal(g["dist_std"], std)
    assert np.allclose(g["sigma_points"][0], mean) and np.allclose(g["sigma_points"][1:P + 1] - mean, np.diag(np.sqrt(scale) * std), rtol=1e-5, atol=1e-9)
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "ut_" + name + ".npz")) < 567 * 1024
    assert ("states" in g) == s["states"] == ("costs_mean" in g)
    if s["states"]:
        assert g["states"].shape == (pts, s["S"], s["N"], s["H"] + 1, f["ds"])
        assert elemerr(g["costs_mean"], g["costs"]) >= 10 * float(g["tol_costs"])
        s64 = twin(g, "states")
        # the closed form on the reference's float64 states is its float64 cost; the two other forms are not
        closed = ut_costs(s64, w, f["goal"], f["w_state"], f["w_term"])
        assert elemerr(closed, g["costs_f64"]) < 1e-12, elemerr(closed, g["costs_f64"])
        assert elemerr(ut_costs(s64, w, f["goal"], f["w_state"], f["w_term"], shifted=False), g["costs_off"]) < 1e-5
        assert elemerr(ut_costs(s64, np.full(pts, 1.0 / pts), f["goal"], f["w_state"], f["w_term"]), g["costs_mean"]) < 1e-5
        assert np.array_equal(g["states"][:, :, :, 0], np.broadcast_to(g["state"], g["states"][:, :, :, 0].shape))


@pytest.mark.parametrize("name", TICK_NAMES)
def test_tick_fixture_caps(golden, name):
    g, s = golden("ut_" + name), TICK_BY_TAG[name]
    for q in TICK_QUANT:
        _check_quantity(g, q, per_slice=q in ("costs", "score", "phi", "theta_after"))
    assert (s["N"], s["S"], s["H"]) == (8, 16, 12) and g["eps"].shape == (int(g["K"]), 16, 8, 12, FAMILY[s["family"]]["da"])
    assert int(np.argmax(g["p_weights"])) == int(np.argmax(g["p_weights_f64"]))
    assert np.array_equal(g["a_seq"], g["theta_after"][-1][int(np.argmax(g["p_weights"]))])


@pytest.mark.parametrize("name", SIGMA_NAMES)
def test_filter_sigma_fixture_caps_and_power(golden, name):
    g, s = golden("ut_sigma_mpf_" + name), SIGMA_BY_TAG[name]
    _check_quantity(g, "points")
    assert elemerr(g["points_nobw"], g["points"]) >= 10 * float(g["tol_points"])
    assert np.array_equal(g["x"], sigma_particles(s)) and g["points"].shape == (2 * s["P"] + 1, s["P"])
    # float64 numpy: mean and bw^2 + population variance of the particles, then mean +- sqrt(scale var) e_p
    x = g["x"].astype(np.float64)
    mean, var = x.mean(0), s["bw"] ** 2 + x.var(0)
    u = np.diag(np.sqrt(float(g["sigma_scale"]) * var))
    assert elemerr(np.concatenate([mean[None], mean + u, mean - u]), g["points_f64"]) < 1e-12
    if s["Mp"] == 1:
        assert np.allclose(var, s["bw"] ** 2)


def test_filter_sigma_fixtures_cover_the_sizes():
    assert {(s["Mp"], s["P"]) for s in SIGMA_BY_TAG.values()} == {(Mp, P) for Mp in SIGMA_SIZES for P in (1, 4)}
    assert SIGMA_SIZES == (1, 2, 63, 64, 257, 1024)


# ---------------------------------------------------------------------------------------------- the C ABI
def test_library_exports_and_declares_the_sigma_point_entries(built):
    from dust_amd import _lib

    lib = C.CDLL(built)
    header = open(os.path.join(ROOT, "include", "dust_amd.h")).read()
    for name in ("dust_mpf_sigma_points", "dust_set_sigma_scale"):
        assert hasattr(lib, name) and name in _lib.SYMBOLS
        assert re.search(r"\bint %s\(" % name, header), name
    assert _lib.SYMBOLS["dust_set_sigma_scale"] == (C.c_int, [_lib.VP, C.c_float])
    assert _lib.SYMBOLS["dust_mpf_sigma_points"] == (C.c_int, [_lib.VP, C.c_float, _lib.FP])


def test_kernels_have_no_spills_and_no_scratch(built, tmp_path):
    llvm = "/opt/rocm/lib/llvm/bin"
    for tool in ("llvm-objdump", "llvm-readelf"):  # (they come with the compiler that built the library)
        assert os.path.exists(llvm + "/" + tool), "%s is missing: the code object cannot be read" % tool
    shutil.copy(built, str(tmp_path / "l.so"))
    subprocess.run([llvm + "/llvm-objdump", "--offloading", "l.so"], cwd=str(tmp_path), check=True, capture_output=True)
    notes = "".join(subprocess.run([llvm + "/llvm-readelf", "--notes", f], cwd=str(tmp_path), check=True, capture_output=True, text=True).stdout
                    for f in os.listdir(str(tmp_path)) if "gfx950" in f)
    want = ("skid_rollout_kernel", "skid_ut_rollout_kernel", "cartpole_rollout_kernel", "cartpole_ut_rollout_kernel", "mpf_sigma_points_kernel")
    found = {}
    for m in re.finditer(r"\.name:\s+(\S+)\n(.*?)\.wavefront_size", notes, re.S):
        for k in want:
            if re.search(r"\d%sE" % k, m.group(1)):  # (the mangled name: length, name, end of the nested name)
                found[k] = (int(re.search(r"\.vgpr_spill_count:\s+(\d+)", m.group(2)).group(1)),
                            int(re.search(r"\.private_segment_fixed_size:\s+(\d+)", m.group(2)).group(1)))
    assert found == {k: (0, 0) for k in want}, found


# ---------------------------------------------------------------------------------------------- the host transform
@pytest.mark.parametrize("n", [1, 2, 3, 4])
def test_host_transform_gives_the_reference_points_and_weights(golden, n):
    from dust_amd.utils.utf import MerweScaledUTF

    name = {1: "cartpole_p1", 2: "cartpole_p2", 3: "skid_p3", 4: "cartpole_p4"}[n]
    g = golden("ut_" + name)
    tf = MerweScaledUTF(n=n, alpha=float(g["alpha"]))
    assert tf.pts == 2 * n + 1 and tf.default_sqrt and abs(tf.scale - float(g["sigma_scale"])) < 1e-12
    assert np.array_equal(tf.loc_weights.numpy(), g["loc_weights"])
    pts = tf.compute_sigma_points(torch.tensor(g["dist_mean"]), torch.diag(torch.tensor(g["dist_std"]) ** 2)).T.numpy()
    assert np.array_equal(pts, g["sigma_points"])
    assert not MerweScaledUTF(n=n, sqrt_method=lambda A: A.sqrt()).default_sqrt
