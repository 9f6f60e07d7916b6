"""Per-environment hyper-parameters in the batched SVMPC tick and its episodes (dust_svmpc_batch_set_hyper / _get_hyper, csrc/svmpc_batch.hpp
svmpc_sweep_kernel, csrc/svmpc_episode.hpp svmpc_sweep_episode_kernel) without a device: the C ABI's two entries and the struct they take,
the Python layers that name them, the register allocation of the eight new kernel instances, the unchanged allocation of the
existing SVMPC batch / episode / dual-period instances, the refusals of `BatchSVMPC.set_hyper` and `BatchDualSVMPC` that need no device,
and the case table of tests/svmpc_sweep_cases.py."""
import ctypes as C
import os
import re
import shutil
import subprocess
import tempfile

import numpy as np
import pytest
import torch

import __graft_entry__ as entry
import svmpc_sweep_cases as cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (VGPRs, SGPRs, spilled VGPRs, spilled SGPRs, private segment bytes) of every SVMPC batch, episode and dual-period instance the library
# had before the sweep instances came, read from a build of the commit before them: svb_body / svb_episode_body are shared text, and a
# new caller must not move them
BEFORE = {
    "_ZN4dust18svmpc_batch_kernelILi0EEEvNS_14SvmpcBatchArgsE": (141, 106, 0, 374, 0),
    "_ZN4dust18svmpc_batch_kernelILi1EEEvNS_14SvmpcBatchArgsE": (134, 106, 0, 400, 0),
    "_ZN4dust18svmpc_batch_kernelILi2EEEvNS_14SvmpcBatchArgsE": (138, 106, 0, 376, 0),
    "_ZN4dust18svmpc_batch_kernelILi3EEEvNS_14SvmpcBatchArgsE": (158, 106, 0, 392, 0),
    "_ZN4dust20svmpc_episode_kernelILi0EEEvNS_16SvmpcEpisodeArgsE": (178, 106, 0, 393, 0),
    "_ZN4dust20svmpc_episode_kernelILi1EEEvNS_16SvmpcEpisodeArgsE": (175, 106, 0, 455, 0),
    "_ZN4dust20svmpc_episode_kernelILi2EEEvNS_16SvmpcEpisodeArgsE": (190, 106, 0, 403, 0),
    "_ZN4dust20svmpc_episode_kernelILi3EEEvNS_16SvmpcEpisodeArgsE": (207, 106, 0, 464, 0),
    "_ZN4dust24svmpc_dual_period_kernelILi0EEEvNS_19SvmpcDualPeriodArgsE": (160, 106, 0, 392, 0),
    "_ZN4dust24svmpc_dual_period_kernelILi1EEEvNS_19SvmpcDualPeriodArgsE": (153, 106, 0, 438, 0),
    "_ZN4dust24svmpc_prior_batch_kernelILi0EEEvNS_19SvmpcPriorBatchArgsE": (158, 106, 0, 373, 0),
    "_ZN4dust24svmpc_prior_batch_kernelILi1EEEvNS_19SvmpcPriorBatchArgsE": (150, 106, 0, 372, 0),
    "_ZN4dust24svmpc_prior_batch_kernelILi2EEEvNS_19SvmpcPriorBatchArgsE": (156, 106, 0, 362, 0),
    "_ZN4dust24svmpc_prior_batch_kernelILi3EEEvNS_19SvmpcPriorBatchArgsE": (178, 106, 0, 368, 0),
    "_ZN4dust27svmpc_skid_nav_batch_kernelENS_17SvmpcNavBatchArgsE": (158, 106, 0, 360, 0),
    "_ZN4dust29svmpc_skid_nav_episode_kernelENS_19SvmpcNavEpisodeArgsE": (195, 106, 0, 455, 0),
    "_ZN4dust33svmpc_skid_nav_prior_batch_kernelENS_22SvmpcNavPriorBatchArgsE": (174, 106, 0, 412, 0),
}
# the substrings by which the existing tests count kernels
OLD_NAMES = ("svmpc_batch_kernel", "svmpc_prior_batch_kernel", "svmpc_episode_kernel", "svmpc_skid_nav_batch_kernel",
             "svmpc_skid_nav_prior_batch_kernel", "svmpc_skid_nav_episode_kernel", "svmpc_dual_period_kernel")
ENTRIES = ("dust_svmpc_batch_set_hyper", "dust_svmpc_batch_get_hyper")


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


def test_library_declares_exports_and_binds_both_entries(built):
    from dust_amd import _lib

    lib = C.CDLL(built)
    header = open(os.path.join(ROOT, "include", "dust_amd.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    for name in ENTRIES:
        assert re.search(r"\b%s\s*\(" % name, code), name + " is not declared"
        assert hasattr(lib, name), name + " is not exported"
        assert name in _lib.SYMBOLS, name + " is not bound"
        assert _lib.SYMBOLS[name] == (C.c_int, [_lib.VP, C.POINTER(_lib.SvmpcHyper)])
    # the header comment cites what the entries replace
    assert "demo/pendulum_tuning.py:30-143" in header and "demo/particle_tuning.py:27-99" in header
    # additive: the version and the profile counters stay where they were
    assert _lib.load().dust_abi_version() == _lib.ABI_VERSION == 3 and "#define DUST_ABI_VERSION 3" in header
    assert _lib.K_ALL == 10


def test_hyper_struct_matches_header():
    """sizeof and every field offset of dust_svmpc_hyper from a C compile against include/dust_amd.h equal the ctypes mirror's"""
    from dust_amd import _lib

    fields = [n for n, _ in _lib.SvmpcHyper._fields_]
    assert fields == ["lr", "alpha", "temperature", "sigma_a", "chol_a", "sigma_p", "weighted_prior"]
    src = '#include "dust_amd.h"\n#include <stdio.h>\n#include <stddef.h>\nint main(){printf("%zu", sizeof(dust_svmpc_hyper));\n' + \
          "".join('printf(" %%zu", offsetof(dust_svmpc_hyper, %s));\n' % f for f in fields) + "return 0;}\n"
    with tempfile.TemporaryDirectory() as d:
        p = os.path.join(d, "p.c")
        open(p, "w").write(src)
        subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), p, "-o", os.path.join(d, "p")], check=True)
        out = subprocess.run([os.path.join(d, "p")], check=True, capture_output=True, text=True).stdout.split()
    S = _lib.SvmpcHyper
    assert [int(v) for v in out] == [C.sizeof(S)] + [getattr(S, f).offset for f in fields]
    assert S.sigma_a.size == 8 and S.lr.size == 8 and C.sizeof(S) == 48


def test_the_python_layers_name_the_rows():
    import dust_amd
    from dust_amd.inference import BatchSVMPC

    assert callable(getattr(dust_amd.SvmpcBatch, "set_hyper", None)) and callable(getattr(dust_amd.SvmpcBatch, "get_hyper", None))
    assert callable(getattr(BatchSVMPC, "set_hyper", None)) and isinstance(BatchSVMPC.hyper, property)
    assert set(dust_amd.SvmpcBatch.HYPER_FIELDS) == set(cases.FIELDS)
    for f in ("examples/svmpc_sweep_example.py", "tools/svmpc_sweep_time.py"):
        assert os.path.exists(os.path.join(ROOT, f)), f


def test_sweep_kernels_do_not_spill(kernels):
    """four instances of svmpc_sweep_kernel and four of svmpc_sweep_episode_kernel, each without VGPR spill or scratch, within the 256
    VGPRs of a 512-lane workgroup; none caught by the substrings the existing tests count kernels by"""
    tick = {k: v for k, v in kernels.items() if "svmpc_sweep_kernel" in k}
    epi = {k: v for k, v in kernels.items() if "svmpc_sweep_episode_kernel" in k}
    assert len(tick) == 4 and len(epi) == 4, (sorted(tick), sorted(epi))
    assert {k: v for k, v in kernels.items() if "sweep" in k} == dict(tick, **epi)
    for k, (vgprs, sgprs, spill, sspill, scratch) in list(tick.items()) + list(epi.items()):
        print(k, "vgprs", vgprs, "sgprs", sgprs, "spill", spill, "scratch", scratch)
        assert spill == 0 and scratch == 0 and vgprs <= 256, (k, spill, scratch, vgprs)
    for old in OLD_NAMES:
        assert not any(old in k for k in list(tick) + list(epi)), old


def test_existing_svmpc_batch_kernels_keep_their_registers(kernels):
    """every instance from before the sweep is still there with the register figures it had: batch x 4, prior batch x 4, the two
    navigation batch kernels, episode x 4, the navigation episode kernel, dual period x 2"""
    assert len(BEFORE) == 4 + 4 + 2 + 4 + 1 + 2
    mine = {k: v for k, v in kernels.items() if any(old in k for old in OLD_NAMES)}
    assert set(mine) == set(BEFORE), sorted(set(mine) ^ set(BEFORE))
    for k, want in BEFORE.items():
        assert mine[k] == want, (k, mine[k], want)


# ------------------------------------------------------------------------------------------------ the class, no device
def _mirror(n_envs, da=1, optimizer_class=torch.optim.SGD, **opt):
    from dust_amd.controllers import MultiDISCO
    from dust_amd.costs import PendulumQuadCos
    from dust_amd.inference import BatchSVMPC, ExponentiatedUtility, get_gmm
    from dust_amd.kernels import RBFKernel
    from dust_amd.models import PendulumModel

    N, S, H = 3, 16, 6
    model, cost = PendulumModel(uncertain_params=("length", "mass")), PendulumQuadCos()
    ctrl = MultiDISCO(model.observation_space, model.action_space, H, N, S, temperature=2.0, a_cov=4.0 * torch.eye(1), inst_cost_fn=cost.inst_cost,
                      term_cost_fn=cost.term_cost, params_sampling=True, params_samples=2)
    mu = torch.zeros(N, H, 1)
    prior = get_gmm(mu, torch.ones(N), 2.25 * torch.eye(1))
    lik = ExponentiatedUtility(alpha=0.5, n_samples=S, controller=ctrl, model=model)
    return BatchSVMPC(n_envs, init_particles=mu, prior=prior, likelihood=lik, kernel=RBFKernel(), n_particles=N, n_steps=1,
                      optimizer_class=optimizer_class, **dict(dict(lr=0.3), **opt))


def test_set_hyper_builds_rows_and_refuses_before_any_device_call():
    B = 3
    sv = _mirror(B)
    h = sv.hyper  # the controller's own values
    assert np.array_equal(h["lr"], np.full(B, float(np.float32(0.3)))) and h["lr"].dtype == np.float64  # plain SGD: dust_config's fp32 lr
    assert np.array_equal(h["alpha"], np.full(B, 0.5, np.float32)) and np.array_equal(h["temperature"], np.full(B, 2.0, np.float32))
    assert np.array_equal(h["sigma_a"], np.full((B, 1), 2.0, np.float32)) and np.array_equal(h["chol_a"], h["sigma_a"])
    assert np.array_equal(h["sigma_p"], np.full((B, 1), 1.5, np.float32)) and not h["weighted_prior"].any()
    sv.set_hyper(lr=[0.1, 1.0, 10.0], alpha=3.0, ctrl_sigma=torch.tensor([[0.5], [1.0], [2.0]]), weighted_prior=[True, False, True])
    h = sv.hyper
    assert np.array_equal(h["lr"], np.array([0.1, 1.0, 10.0], np.float32).astype(np.float64))
    assert np.array_equal(h["alpha"], np.full(B, 3.0, np.float32)) and np.array_equal(h["temperature"], np.full(B, 2.0, np.float32))  # independent
    assert np.array_equal(h["sigma_a"][:, 0], [0.5, 1.0, 2.0]) and np.array_equal(h["chol_a"], h["sigma_a"])  # diagonal: cholesky = sigma
    assert np.array_equal(h["sigma_p"], np.full((B, 1), 1.5, np.float32)) and np.array_equal(h["weighted_prior"], [1, 0, 1])
    kept = {k: v.copy() for k, v in h.items()}
    for kw in (dict(lr=[0.1, 0.2]), dict(alpha=np.ones((3, 1))), dict(prior_sigma=np.ones((3, 2))), dict(ctrl_sigma=np.ones((2, 1))),
               dict(lr=0.0), dict(lr=[0.1, -1.0, 1.0]), dict(alpha=float("nan")), dict(temperature=float("inf")), dict(prior_sigma=[1.0, 0.0, 1.0]),
               dict(ctrl_sigma=-1.0), dict(weighted_prior=2), dict(weighted_prior=[0, 1, 0.5]), dict(lr=1e-60)):
        with pytest.raises(ValueError):
            sv.set_hyper(**kw)
        assert all(np.array_equal(sv.hyper[k], v) for k, v in kept.items()), kw  # a refused call leaves the rows as they were
    assert sv._batch is None  # nothing was created: no device call has been made
    import copy

    twin = copy.deepcopy(sv)
    assert all(np.array_equal(twin.hyper[k], v) for k, v in kept.items()) and twin._hyper is not sv._hyper
    sv.set_hyper()  # every argument None: back to the controller's values
    assert sv._hyper is None and np.array_equal(sv.hyper["alpha"], np.full(B, 0.5, np.float32))
    # an optimiser beyond dust_config's plain ones carries its lr in double
    mom = _mirror(2, momentum=0.9)
    mom.set_hyper(lr=[0.1, 0.3])
    assert np.array_equal(mom.hyper["lr"], [0.1, 0.3])


def test_batch_dual_svmpc_refuses_rows_before_any_device_call():
    from dust_amd.controllers import BatchDualSVMPC

    sv = _mirror(2)
    sv.set_hyper(lr=[0.1, 0.2])

    class Filter:
        draw_source = None

    with pytest.raises(NotImplementedError, match="per-environment hyper-parameters"):
        BatchDualSVMPC(sv, Filter())
    dual = BatchDualSVMPC.__new__(BatchDualSVMPC)  # rows set on the controller of an existing loop
    dual.svmpc, dual.n_steps, dual.mpf = sv, None, Filter()
    with pytest.raises(NotImplementedError, match="per-environment hyper-parameters"):
        dual.forward(torch.zeros(2, 2))
    with pytest.raises(NotImplementedError, match="per-environment hyper-parameters"):
        dual.run_episodes(torch.zeros(2, 2), 2)
    assert sv._batch is None


# ------------------------------------------------------------------------------------------------ the case table
def test_the_case_table_is_what_the_issue_sets():
    by = cases.BY_ID
    assert cases.IDS == ["pend", "part", "skid", "cart", "ones", "corner"] and cases.EPISODE_IDS == ["pend", "part", "ones"] and cases.T_EPISODE == 4
    shape = lambda c: (c["family"], c["N"], c["S"], c["M"], c["H"])
    assert shape(by["pend"]) == ("pendulum", 3, 32, 2, 8) and by["pend"]["opts"] == dict(optimizer="SGD", kernel="K1")
    assert set(by["pend"]["iters"]) == {1, 3} and cases.n_params(by["pend"]) == 2
    assert shape(by["part"]) == ("particle", 4, 16, 1, 6) and by["part"]["opts"] == dict(optimizer="Adam", kernel="IMQ", roll_strategy="mean")
    assert shape(by["skid"]) == ("skid_steer", 2, 8, 2, 5) and by["skid"]["opts"]["optimizer"] == "SGD"
    assert shape(by["cart"]) == ("cartpole", 2, 8, 1, 5) and by["cart"]["opts"]["optimizer"] == "Adam"
    assert shape(by["ones"]) == ("pendulum", 1, 1, 1, 1) and by["ones"]["B"] == 2
    assert shape(by["corner"]) == ("particle", 64, 4, 1, 64) and by["corner"]["H"] * cases.family(by["corner"])["da"] == 128
    assert all(c["B"] == 5 for c in cases.CASES if c["id"] != "ones")
    r = cases.base_row(by["part"])  # two channels with different sigmas inside a row
    assert r["sigma_a"][0] != r["sigma_a"][1] and r["sigma_p"][0] != r["sigma_p"][1]


@pytest.mark.parametrize("cid", cases.IDS)
def test_rows_are_valid_and_pairwise_distinct(cid):
    case = cases.BY_ID[cid]
    rows, base = cases.env_rows(case), cases.base_row(case)
    assert len(rows) == case["B"] and base["alpha"] == 1.0 and base["temperature"] == 1.0
    for r in rows:
        assert np.isfinite(r["lr"]) and r["lr"] > 0 and r["alpha"] > 0 and r["temperature"] > 0 and r["weighted_prior"] in (0, 1)
        for k in ("sigma_a", "chol_a", "sigma_p"):
            assert r[k].dtype == np.float32 and r[k].shape == (cases.family(case)["da"],) and np.isfinite(r[k]).all() and (r[k] > 0).all()
        assert float(np.float32(r["lr"])) == r["lr"]  # what a prototype Context built with the row carries
    for i in range(len(rows)):
        for j in range(i + 1, len(rows)):
            assert not cases.row_equal(rows[i], rows[j]), (i, j)
    if case["B"] == 5:
        assert cases.row_equal(rows[0], base) and rows[1]["lr"] == 4 * base["lr"]
        assert rows[2]["alpha"] * rows[2]["temperature"] == 1.0 and (rows[2]["alpha"], rows[2]["temperature"]) == (0.5, 2.0)
        assert rows[3]["alpha"] * rows[3]["temperature"] != 1.0 and (rows[3]["alpha"], rows[3]["temperature"]) == (2.0, 1.5)
        assert np.array_equal(rows[4]["sigma_a"], base["sigma_a"] * np.float32(1.5)) and np.array_equal(rows[4]["chol_a"], rows[4]["sigma_a"])
        assert np.array_equal(rows[4]["sigma_p"], base["sigma_p"] * np.float32(0.5)) and rows[4]["weighted_prior"] == 1 - base["weighted_prior"]
    st = cases.stack(rows)
    assert st["lr"].dtype == np.float64 and st["sigma_a"].shape == (case["B"], cases.family(case)["da"])


@pytest.mark.parametrize("field", list(cases.VARIANTS))
def test_every_variant_changes_its_field_alone(field):
    for cid in ("pend", "part"):
        for r in cases.env_rows(cases.BY_ID[cid]):
            v = cases.VARIANTS[field][0](r)
            assert not cases.row_equal(v, r)
            moved = {k for k in cases.FIELDS if not np.array_equal(np.asarray(v[k]), np.asarray(r[k]))}
            assert moved == ({"sigma_a", "chol_a"} if field == "sigma_a" else {field}), (field, moved)
            assert np.all(np.asarray(v["lr"]) > 0) and v["alpha"] > 0 and v["temperature"] > 0 and (v["sigma_p"] > 0).all()


def test_context_keywords_carry_a_row():
    case = cases.BY_ID["part"]
    r = cases.env_rows(case)[4]
    kw = cases.context_kwargs(case, r)
    assert kw["lr"] == r["lr"] and kw["alpha"] == 1.0 and np.array_equal(kw["sigma_a"], r["sigma_a"]) and np.array_equal(kw["chol_a"], r["chol_a"])
    assert np.array_equal(kw["sigma_p"], r["sigma_p"]) and kw["weighted_prior"] is True and kw["roll_strategy"] == "mean" and kw["kernel"] == "IMQ"
    inp = cases.env_inputs(case)
    assert inp["th"].shape == (5, 4, 6, 2) and inp["params"][0] is None and inp["plant"] is None and len(set(inp["seeds"])) == 5
    pend = cases.env_inputs(cases.BY_ID["pend"])
    assert pend["params"][1].shape == (5, 3, 2, 2) and pend["ep_params"].shape == (5, 5, 1, 2, 2) and pend["plant"].shape == (5, 2)
