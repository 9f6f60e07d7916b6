"""AMPPI without a device: the fixtures' own conditions (tests/golden/amppi_*.npz, generator tests/golden/make_golden_amppi.py), the
float64 restatement of the tick's arithmetic (tests/amppi_cases.py restate) against every fixture's float64 twin, the new kernel's
register allocation, the C ABI's new entries and the refusals that need no device."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import __graft_entry__ as entry
import amppi_cases as cases
from helpers import elemerr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def built():
    return entry.build()


def _grid(s):
    if s["family"] != "particle":
        return None
    from oracle import grid_4x4_map

    return grid_4x4_map()


def _variants(g):
    return [k for k in g if k.startswith("costs_") and k != "costs_f64"]


@pytest.mark.parametrize("name", cases.NAMES)
def test_fixture_conditions(golden, name):
    """tolerances = max(1e-5, 2 d) under the cap; for S > 2 the largest weight <= 0.5; the update moves a_seq by >= 100 tolerances; every
    power variant >= 10 tolerances from the true quantity; the inputs are the cases file's"""
    s, g = cases.BY_TAG[name], golden("amppi_" + name)
    quant = cases.QUANT + (("states",) if s["states"] else ())
    for q in quant:
        tol = float(g["tol_" + q])
        assert cases.TOL <= tol <= cases.CAP, (q, tol)
        assert elemerr(g[q], cases.twin(g, q)) <= tol / 2 * (1 + 1e-6), q  # (2 d with d >= the fp32 / float64 distance)
    assert ("states" in g) == s["states"]
    if s["S"] > 2:
        assert float(np.exp(g["omega"]).max()) <= 0.5
    assert abs(float(np.exp(g["omega"].astype(np.float64)).sum()) - 1.0) < 1e-5
    assert elemerr(g["a_seq1"], g["a_seq0"]) >= 100 * float(g["tol_a_seq1"])
    want = {"costs_disco", "costs_noctrl"} | ({"costs_single"} if s["mode"] == "extended" else set()) | ({"costs_mean"} if s["mode"] == "ut" else set())
    assert set(_variants(g)) == want
    for v in want:
        assert elemerr(g[v], g["costs"]) >= 10 * float(g["tol_costs"]), v
    if s.get("a_seq0") == "edge":
        assert elemerr(g["a_seq1_noclamp"], g["a_seq1"]) >= 10 * float(g["tol_a_seq1"])
    for k, v in cases.inputs(s).items():
        assert np.array_equal(g[k], v), k
    f = cases.FAMILY[s["family"]]
    assert float(g["lam"]) == f["lam"] and int(g["S"]) == s["S"] and int(g["H"]) == s["H"] and str(g["mode"]) == s["mode"]
    lo, hi = np.asarray(f["lo"], np.float32), np.asarray(f["hi"], np.float32)
    assert (g["a_seq1"] >= lo).all() and (g["a_seq1"] <= hi).all()


def test_loop_fixture_conditions(golden):
    s, g = cases.LOOP, golden("amppi_pend_loop")
    for q in cases.QUANT + ("plant",):
        tol = np.asarray(g["tol_" + q])
        assert tol.shape == (s["ticks"],) and (tol >= cases.TOL).all() and (tol <= cases.CAP).all(), q
    assert float(np.exp(g["omega"]).max()) <= 0.5
    for v in cases.LOOP_VARIANTS:
        for k in range(s["ticks"]):
            assert elemerr(g["costs_" + v][k], g["costs"][k]) >= 10 * float(g["tol_costs"][k]), (v, k)
    inp = cases.loop_inputs(s)
    for k in ("state", "a_seq0", "params"):
        assert np.array_equal(g[k], inp[k]), k
    # the recorded actions of tick 0 are a_seq0 + sigma_a z; the later ones were drawn around the sequence the reference had then
    assert np.array_equal(g["actions"][0], (inp["a_seq0"][None] + np.float32(cases.PEND["sigma_a"]) * inp["z"][0]).astype(np.float32))


@pytest.mark.parametrize("name", cases.NAMES)
def test_restatement_is_the_float64_twin(golden, name):
    """section 1 of the tick in float64 numpy (amppi_cases.restate) reproduces the reference's float64 run to 1e-12 - and its variants
    are the fixture's power variants"""
    s, g = cases.BY_TAG[name], golden("amppi_" + name)
    grid, sp = _grid(s), (g["sigma_points"] if s["mode"] == "ut" else None)
    r = cases.restate(s, g, grid=grid, sigma_points=sp)
    for q in cases.QUANT + (("states",) if s["states"] else ()):
        assert elemerr(r[q], cases.twin(g, q)) < 1e-12, q
    for v in _variants(g):
        rv = cases.restate(s, g, variant=v[len("costs_"):], grid=grid, sigma_points=sp)["costs"]
        assert np.array_equal(rv.astype(np.float32), g[v]), v
    if s["mode"] == "ut":
        n = len(s["up"])
        assert np.allclose(g["loc_weights"], cases.weights(n)[0], rtol=1e-6) and g["sigma_points"].shape == (2 * n + 1, n)
        assert np.array_equal(g["sigma_points"][0], g["dist_mean"])


def test_loop_restatement_is_the_float64_twin(golden):
    s, g = cases.LOOP, golden("amppi_pend_loop")
    r = cases.restate_loop(s, g)
    for q in cases.QUANT + ("plant",):
        assert elemerr(r[q], g[q + "_f64"]) < 1e-12, q
    for v, c in cases.restate_loop_variants(s, g, g["a_seq1_f64"], g["plant_f64"]).items():
        assert np.array_equal(c.astype(np.float32), g[v]), v


def test_fixture_files_are_small():
    for n in cases.NAMES + [cases.LOOP["tag"]]:
        assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "amppi_" + n + ".npz")) < 512 * 1024, n


# ---------------------------------------------------------------------------------------------- the library
def test_library_exports_and_binds_the_amppi_entries(built):
    from dust_amd import _lib

    lib = C.CDLL(built)
    for name in ("dust_amppi_update", "dust_amppi_roll"):
        assert hasattr(lib, name) and name in _lib.SYMBOLS
    assert _lib.load().dust_abi_version() == _lib.ABI_VERSION == 3
    assert _lib.load().dust_kernel_name(_lib.K_AMPPI) == b"amppi_kernel" and _lib.K_COUNT == _lib.K_AMPPI + 1
    header = open(os.path.join(ROOT, "include", "dust_amd.h")).read()
    assert "#define DUST_ABI_VERSION 3" in header and "DUST_K_AMPPI = 8" in header and "DUST_AMPPI_PARAMS_SHARED = 32" in header
    assert _lib.AMPPI_PARAMS_SHARED == 32


def test_amppi_kernels_do_not_spill(built, tmp_path):
    """the method of test_hot_kernels_do_not_spill: the gfx950 code object's metadata shows no VGPR spill and no scratch for the four
    instances of amppi_kernel"""
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
    mine = {k: v for k, v in kernels.items() if "amppi_kernel" in k}
    assert len(mine) == 4, sorted(mine)
    for k, (spill, scratch, vgprs) in mine.items():
        assert spill == 0 and scratch == 0 and vgprs <= 128, (k, spill, scratch, vgprs)


# ---------------------------------------------------------------------------------------------- refusals that need no device
def _pend():
    from dust_amd.costs import PendulumQuadCos
    from dust_amd.models import PendulumModel

    return PendulumModel(uncertain_params=("length",)), PendulumQuadCos()


def test_constructor_follows_the_reference():
    import torch

    from dust_amd.controllers import AMPPI
    from dust_amd.utils.utf import MerweScaledUTF

    m, c = _pend()
    kw = dict(inst_cost_fn=c.inst_cost, term_cost_fn=c.term_cost)
    with pytest.raises(ValueError, match="Invalid value for 'params_sampling': all"):
        AMPPI(m.observation_space, m.action_space, 8, 64, params_sampling="all", **kw)
    with pytest.raises(ValueError, match="Specify at least one cost function"):
        AMPPI(m.observation_space, m.action_space, 8, 64)
    tf = MerweScaledUTF(n=1)
    for ps in ("none", "single", "extended", None, False, tf):
        assert AMPPI(m.observation_space, m.action_space, 8, 64, params_sampling=ps, **kw).params_sampling is ps
    a = AMPPI(m.observation_space, m.action_space, 8, 64, lambda_=3.0, a_cov=4.0 * torch.eye(1), **kw)
    assert a.params_sampling == "extended" and a.lambda_ == 3.0 and a.n_samples == 64 and a.hz_len == 8 and a.dim_a == 1 and a.dim_s == 2
    assert float(a.a_pre) == 0.25 and not a.a_seq.any() and tuple(a.a_seq.shape) == (8, 1) and a.return_rollouts
    init = torch.arange(8.0).view(8, 1)
    b = AMPPI(m.observation_space, m.action_space, 8, 64, init_actions=init, **kw)  # (a tensor: the reference's `if not init_actions` raises)
    assert torch.equal(b.a_seq, init)
    b.roll(3)  # before any device context: on the host
    assert torch.equal(b.a_seq[:5], init[3:]) and not b.a_seq[5:].any()
    b.roll(20)
    assert not b.a_seq.any()
    with pytest.raises(ValueError):
        b.roll(0)
    with pytest.raises(NotImplementedError, match="dim_a = 2"):
        AMPPI(m.observation_space, m.action_space, 8, 64, a_cov=torch.tensor([[1.0, 0.5], [0.5, 1.0]]), **kw)


def test_refusals_before_any_device_call():
    import torch

    from dust_amd.controllers import AMPPI
    from dust_amd.costs import QuadraticCost
    from dust_amd.models import CartPoleModel, Particle

    m, c = _pend()
    kw = dict(inst_cost_fn=c.inst_cost, term_cost_fn=c.term_cost)
    state = torch.tensor([3.0, 0.0])

    class Other:
        family = "walker"

    with pytest.raises(NotImplementedError, match="no AMPPI kernel family"):
        AMPPI(m.observation_space, m.action_space, 8, 64, **kw).update_actions(Other(), state)
    with pytest.raises(NotImplementedError, match="128"):
        AMPPI(m.observation_space, m.action_space, 129, 64, params_sampling="none", **kw).update_actions(m, state)
    with pytest.raises(NotImplementedError, match="65536"):
        AMPPI(m.observation_space, m.action_space, 8, 65537, params_sampling="none", **kw).update_actions(m, state)
    with pytest.raises(NotImplementedError):  # an opaque cost callable
        AMPPI(m.observation_space, m.action_space, 8, 64, inst_cost_fn=lambda x: x.sum(-1), term_cost_fn=c.term_cost,
              params_sampling="none").update_actions(m, state)
    cart = CartPoleModel()
    qc = QuadraticCost((0, 0, 0, 0), (1, 1, 1, 1), w_ctrl=(0.1,))
    with pytest.raises(NotImplementedError, match="w_ctrl"):
        AMPPI(cart.observation_space, cart.action_space, 8, 64, inst_cost_fn=qc.inst_cost, term_cost_fn=qc.term_cost,
              params_sampling="none").update_actions(cart, torch.zeros(4))
    with pytest.raises(ValueError, match="uncertain_params"):  # sampling without uncertain parameters
        q0 = QuadraticCost((0, 0, 0, 0), (1, 1, 1, 1))
        AMPPI(cart.observation_space, cart.action_space, 8, 64, inst_cost_fn=q0.inst_cost, term_cost_fn=q0.term_cost).update_actions(cart, torch.zeros(4))
    many = CartPoleModel(uncertain_params=("g", "length", "mass_pole", "mass_cart", "f_mag"))
    q0 = QuadraticCost((0, 0, 0, 0), (1, 1, 1, 1))
    with pytest.raises(NotImplementedError, match="at most 4"):
        AMPPI(many.observation_space, many.action_space, 8, 64, inst_cost_fn=q0.inst_cost, term_cost_fn=q0.term_cost).update_actions(many, torch.zeros(4))
    noisy = Particle(**dict(cases.PART_ENV, deterministic=False), mass=2.0)
    with pytest.raises(NotImplementedError, match="deterministic"):
        AMPPI(noisy.observation_space, noisy.action_space, 8, 64, inst_cost_fn=noisy.default_inst_cost, term_cost_fn=noisy.default_term_cost,
              params_sampling="none").update_actions(noisy, torch.zeros(4))


def test_base_model_draws_parameters_as_the_reference():
    """BaseModel.params_dist / rejection_sampling / sample_params (base.py:102-171) and the alias AMPPI's sigma branch calls"""
    import torch
    import torch.distributions as dist

    from dust_amd.models import CartPoleModel, PendulumModel

    m = PendulumModel(uncertain_params=("mass", "length"))
    assert m.params_dist is None
    with pytest.raises(AssertionError, match="No sampling distribution"):
        m.sample_params(4)
    m.params_dist = dist.MultivariateNormal(torch.tensor([1.0, 1.0]), covariance_matrix=0.01 * torch.eye(2))
    torch.manual_seed(3)
    d = m.sample_params(50, x_min=0.95, x_max=1.2)
    assert list(d) == ["mass", "length"] and all(tuple(v.shape) == (50, 1) for v in d.values())
    assert all(bool(((v > 0.95) & (v < 1.2)).all()) for v in d.values())
    samples, attempts = m.rejection_sampling(50, x_min=0.95, x_max=1.2)
    assert tuple(samples.shape) == (50, 2) and attempts > 1
    torch.manual_seed(4)
    a = m.sample_params(7)
    torch.manual_seed(4)
    assert torch.equal(m.dict_to_params(a), m.params_dist.sample([7]))  # (without bounds: one draw, handed out as drawn)
    rows = torch.arange(6.0).view(3, 2)
    assert m.to_params_dict.__func__ is m.params_to_dict.__func__ and torch.equal(m.to_params_dict(rows)["length"], rows[:, 1:])
    one = CartPoleModel(uncertain_params=("length",))
    one.params_dist = dist.Normal(torch.tensor([1.0]), torch.tensor([0.1]))  # (event shape [1] by batch)
    assert tuple(one.sample_params(5)["length"].shape) == (5, 1)
    with pytest.raises(AssertionError, match="at least one sample"):
        one.sample_params(0)


def test_generator_dry_table_reproduces_the_stored_tolerances(golden):
    """when the reference tree is present: the committed generator, run dry, gives the stored fixtures again"""
    from oracle import ref_shim

    if not os.path.isdir(os.path.join(ref_shim.REFERENCE_ROOT, "dust")):
        pytest.skip("the reference tree is not on this machine")
    tags = ["pend_one", "pend_ut_65", "cart_ext_255", "skid_none_63", "part_none_64", "pend_loop"]
    code = ("import sys, json, numpy as np; sys.argv = ['x']; sys.path.insert(0, %r); import make_golden_amppi as G; out = {}\n"
            "for t in %r:\n"
            "    s = G.cases.BY_TAG[t]; g = (G.run_loop if 'ticks' in s else G.run)(s, write=False)\n"
            "    out[t] = {k: np.asarray(v, np.float64).reshape(-1).tolist() for k, v in g.items() if k.startswith('tol_')}\n"
            "    out[t]['costs'] = np.asarray(g['costs'], np.float64).reshape(-1)[:8].tolist()\n"
            "print('TABLE' + json.dumps(out))\n") % (os.path.join(ROOT, "tests", "golden"), tags)
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True, check=True)
    import json

    table = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("TABLE")][0][5:])
    for t in tags:
        g = golden("amppi_" + t)
        for k, v in table[t].items():
            want = np.asarray(g[k], np.float64).reshape(-1)
            assert np.array_equal(np.asarray(v), want if k != "costs" else want[:8]), (t, k)
