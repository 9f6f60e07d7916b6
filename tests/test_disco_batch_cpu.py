"""MultiDISCO over a batch of plants (dust_disco_batch_*, csrc/disco_batch.hpp) without a device: the C ABI's new entries and the Python
layers that name them, the register allocation of every new kernel instance, the float64 restatement of tests/disco_cases.py against an
independent torch float64 statement, the power of the checks of tests/test_gpu_disco_batch.py (tolerances and distances from the wrong
forms, from the restatement alone), the forced events of the Particle episode, and the refusals of `BatchDISCO` that need no device."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

import __graft_entry__ as entry
import disco_cases as dc
from helpers import elemerr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = {"dust_disco_batch_create": 4, "dust_disco_batch_destroy": 1, "dust_disco_batch_clone": 2, "dust_disco_batch_ctx": 2,
           "dust_disco_batch_set": 3, "dust_disco_batch_get": 3, "dust_disco_batch_forward": 6, "dust_disco_batch_step": 6,
           "dust_disco_batch_tick": 10, "dust_disco_batch_episode": 16}


@pytest.fixture(scope="module")
def built():
    return entry.build()


def test_library_declares_exports_and_binds_the_entries(built):
    from dust_amd import _lib

    lib = C.CDLL(built)
    header = open(os.path.join(ROOT, "include", "dust_amd.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    for name, n_args in ENTRIES.items():
        assert re.search(r"\b%s\s*\(" % name, code), name + " is not declared"
        assert hasattr(lib, name), name + " is not exported"
        assert name in _lib.SYMBOLS, name + " is not bound"
        assert len(_lib.SYMBOLS[name][1]) == n_args, name
        decl = re.search(r"\b%s\s*\((.*?)\)\s*;" % name, code, re.S).group(1)
        assert len(decl.split(",")) == n_args, (name, decl)
    ep = _lib.SYMBOLS["dust_disco_batch_episode"][1]
    assert ep[6] == C.POINTER(_lib.EpisodeRules) and ep[13] == ep[14] == C.POINTER(C.c_int)
    # additive: the version, the ids and the profile counters stay where they were
    assert _lib.load().dust_abi_version() == _lib.ABI_VERSION == 3 and "#define DUST_ABI_VERSION 3" in header
    assert "DUST_K_SVMPC_BATCH = 9" in code and _lib.K_ALL == 10
    assert "DUST_DISCO_PARAMS_ONCE = 128" in code and _lib.DISCO_PARAMS_ONCE == 128
    flags = (_lib.PTR_DEVICE, _lib.STORE_STATES, _lib.EPS_AROUND_A_MAT, _lib.EPS_F16, _lib.STORE_F16, _lib.AMPPI_PARAMS_SHARED, _lib.SVMPC_BATCH_KEEP_ACTIONS)
    assert all(_lib.DISCO_PARAMS_ONCE & f == 0 for f in flags)
    for k, n in enumerate(("A_MAT", "A_SEQ", "A_MIX", "COSTS", "OMEGA", "ACTIONS")):
        assert getattr(_lib, "DCB_" + n) == k and re.search(r"DUST_DCB_%s = %d\b" % (n, k), code), n


def test_the_python_layers_name_the_batch():
    import dust_amd
    from dust_amd.controllers import BatchDISCO, MultiDISCO

    for m in ("set", "get", "forward", "step", "tick", "episode", "clone"):
        assert callable(getattr(dust_amd.DiscoBatch, m, None)), m
    assert callable(getattr(dust_amd.Context, "disco_batch", None))
    for m in ("forward", "step", "tick", "run_episodes", "simulate"):
        assert callable(getattr(BatchDISCO, m, None)), m
    assert issubclass(BatchDISCO, MultiDISCO)


def _kernel_figures(built, tmp_path):
    """name -> (vgpr spill, private segment, vgprs) of the gfx950 code object (the method of tests/test_svmpc_batch_cpu.py)"""
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


# VGPRs of every batched SVMPC / AMPPI kernel instance (tick, episode, sim, sweep, dual period; no spill, no scratch), read from the code
# object of the commit before the batched MultiDISCO: the new body sits beside them in one translation unit and must not move them
PARENT_VGPRS = {
    "_ZN4dust16svmpc_sim_kernelILi0EEEvNS_12SvmpcSimArgsE": 180,
    "_ZN4dust16svmpc_sim_kernelILi1EEEvNS_12SvmpcSimArgsE": 177,
    "_ZN4dust16svmpc_sim_kernelILi2EEEvNS_12SvmpcSimArgsE": 191,
    "_ZN4dust16svmpc_sim_kernelILi3EEEvNS_12SvmpcSimArgsE": 208,
    "_ZN4dust18amppi_batch_kernelILi0EEEvNS_14AmppiBatchArgsE": 51,
    "_ZN4dust18amppi_batch_kernelILi1EEEvNS_14AmppiBatchArgsE": 47,
    "_ZN4dust18amppi_batch_kernelILi2EEEvNS_14AmppiBatchArgsE": 52,
    "_ZN4dust18amppi_batch_kernelILi3EEEvNS_14AmppiBatchArgsE": 66,
    "_ZN4dust18svmpc_batch_kernelILi0EEEvNS_14SvmpcBatchArgsE": 141,
    "_ZN4dust18svmpc_batch_kernelILi1EEEvNS_14SvmpcBatchArgsE": 134,
    "_ZN4dust18svmpc_batch_kernelILi2EEEvNS_14SvmpcBatchArgsE": 138,
    "_ZN4dust18svmpc_batch_kernelILi3EEEvNS_14SvmpcBatchArgsE": 158,
    "_ZN4dust18svmpc_sweep_kernelILi0EEEvNS_14SvmpcSweepArgsE": 140,
    "_ZN4dust18svmpc_sweep_kernelILi1EEEvNS_14SvmpcSweepArgsE": 134,
    "_ZN4dust18svmpc_sweep_kernelILi2EEEvNS_14SvmpcSweepArgsE": 138,
    "_ZN4dust18svmpc_sweep_kernelILi3EEEvNS_14SvmpcSweepArgsE": 158,
    "_ZN4dust19amppi_period_kernelILi0EEEvNS_15AmppiPeriodArgsE": 51,
    "_ZN4dust19amppi_period_kernelILi1EEEvNS_15AmppiPeriodArgsE": 47,
    "_ZN4dust19amppi_period_kernelILi2EEEvNS_15AmppiPeriodArgsE": 52,
    "_ZN4dust19amppi_period_kernelILi3EEEvNS_15AmppiPeriodArgsE": 66,
    "_ZN4dust20svmpc_episode_kernelILi0EEEvNS_16SvmpcEpisodeArgsE": 178,
    "_ZN4dust20svmpc_episode_kernelILi1EEEvNS_16SvmpcEpisodeArgsE": 175,
    "_ZN4dust20svmpc_episode_kernelILi2EEEvNS_16SvmpcEpisodeArgsE": 190,
    "_ZN4dust20svmpc_episode_kernelILi3EEEvNS_16SvmpcEpisodeArgsE": 207,
    "_ZN4dust21svmpc_rows_sim_kernelILi0EEEvNS_16SvmpcRowsSimArgsE": 180,
    "_ZN4dust21svmpc_rows_sim_kernelILi1EEEvNS_16SvmpcRowsSimArgsE": 177,
    "_ZN4dust21svmpc_rows_sim_kernelILi2EEEvNS_16SvmpcRowsSimArgsE": 191,
    "_ZN4dust21svmpc_rows_sim_kernelILi3EEEvNS_16SvmpcRowsSimArgsE": 208,
    "_ZN4dust24amppi_prior_batch_kernelILi0EEEvNS_19AmppiPriorBatchArgsE": 40,
    "_ZN4dust24amppi_prior_batch_kernelILi1EEEvNS_19AmppiPriorBatchArgsE": 35,
    "_ZN4dust24amppi_prior_batch_kernelILi2EEEvNS_19AmppiPriorBatchArgsE": 42,
    "_ZN4dust24amppi_prior_batch_kernelILi3EEEvNS_19AmppiPriorBatchArgsE": 52,
    "_ZN4dust24svmpc_dual_period_kernelILi0EEEvNS_19SvmpcDualPeriodArgsE": 160,
    "_ZN4dust24svmpc_dual_period_kernelILi1EEEvNS_19SvmpcDualPeriodArgsE": 153,
    "_ZN4dust24svmpc_prior_batch_kernelILi0EEEvNS_19SvmpcPriorBatchArgsE": 158,
    "_ZN4dust24svmpc_prior_batch_kernelILi1EEEvNS_19SvmpcPriorBatchArgsE": 150,
    "_ZN4dust24svmpc_prior_batch_kernelILi2EEEvNS_19SvmpcPriorBatchArgsE": 156,
    "_ZN4dust24svmpc_prior_batch_kernelILi3EEEvNS_19SvmpcPriorBatchArgsE": 178,
    "_ZN4dust25amppi_prior_period_kernelILi0EEEvNS_20AmppiPriorPeriodArgsE": 40,
    "_ZN4dust25amppi_prior_period_kernelILi1EEEvNS_20AmppiPriorPeriodArgsE": 35,
    "_ZN4dust25svmpc_skid_nav_sim_kernelENS_15SvmpcNavSimArgsE": 195,
    "_ZN4dust26svmpc_sweep_episode_kernelILi0EEEvNS_21SvmpcSweepEpisodeArgsE": 179,
    "_ZN4dust26svmpc_sweep_episode_kernelILi1EEEvNS_21SvmpcSweepEpisodeArgsE": 176,
    "_ZN4dust26svmpc_sweep_episode_kernelILi2EEEvNS_21SvmpcSweepEpisodeArgsE": 192,
    "_ZN4dust26svmpc_sweep_episode_kernelILi3EEEvNS_21SvmpcSweepEpisodeArgsE": 207,
    "_ZN4dust27amppi_skid_nav_batch_kernelENS_17AmppiNavBatchArgsE": 55,
    "_ZN4dust27svmpc_skid_nav_batch_kernelENS_17SvmpcNavBatchArgsE": 158,
    "_ZN4dust28amppi_skid_nav_period_kernelENS_18AmppiNavPeriodArgsE": 55,
    "_ZN4dust28svmpc_dual_sim_period_kernelILi0EEEvNS_22SvmpcDualSimPeriodArgsE": 161,
    "_ZN4dust28svmpc_dual_sim_period_kernelILi1EEEvNS_22SvmpcDualSimPeriodArgsE": 153,
    "_ZN4dust29svmpc_skid_nav_episode_kernelENS_19SvmpcNavEpisodeArgsE": 195,
    "_ZN4dust33amppi_skid_nav_prior_batch_kernelENS_22AmppiNavPriorBatchArgsE": 46,
    "_ZN4dust33svmpc_skid_nav_prior_batch_kernelENS_22SvmpcNavPriorBatchArgsE": 174,
}
assert len(PARENT_VGPRS) == 53


def test_disco_kernels_do_not_spill(built, tmp_path):
    """four plain and three sigma-point instances (Pendulum, skid-steer, cart-pole) of disco_batch_kernel and of disco_episode_kernel, two
    navigation instances of each: every one without VGPR spill or scratch and within 256 VGPRs (512 lanes per workgroup)"""
    kernels = _kernel_figures(built, tmp_path)
    groups = {n: {k: v for k, v in kernels.items() if n in k} for n in
              ("disco_batch_kernel", "disco_episode_kernel", "disco_skid_nav_batch_kernel", "disco_skid_nav_episode_kernel")}
    assert [len(groups[n]) for n in groups] == [7, 7, 2, 2], {n: sorted(v) for n, v in groups.items()}
    for n in ("disco_batch_kernel", "disco_episode_kernel"):
        plain = sorted(re.search(r"ILi(\d)ELb0E", k).group(1) for k in groups[n] if "Lb0E" in k)
        sigma = sorted(re.search(r"ILi(\d)ELb1E", k).group(1) for k in groups[n] if "Lb1E" in k)
        assert plain == ["0", "1", "2", "3"] and sigma == ["0", "2", "3"], (n, plain, sigma)  # (no sigma points for Particle: model 1)
    for g in groups.values():
        for k, (spill, scratch, vgprs) in g.items():
            print(k, "spill", spill, "scratch", scratch, "vgprs", vgprs)
            assert spill == 0 and scratch == 0 and vgprs <= 256, (k, spill, scratch, vgprs)
    # no new kernel hides in the counts the existing tests take by substring, and the existing batched instances are where they were
    new = [k for g in groups.values() for k in g]
    old = ("svmpc_batch_kernel", "svmpc_prior_batch_kernel", "svmpc_skid_nav_batch_kernel", "svmpc_episode_kernel", "svmpc_sim_kernel",
           "svmpc_sweep_kernel", "amppi_batch_kernel", "amppi_episode_kernel")
    for o in old:
        assert not any(o in k for k in new), o
    # ... with the figures they had before this file's kernels joined the unit: every batched SVMPC and AMPPI instance keeps its VGPR count
    for k, vgprs in PARENT_VGPRS.items():
        assert k in kernels, k
        assert kernels[k] == (0, 0, vgprs), (k, kernels[k], vgprs)


# ------------------------------------------------------------------------------------------------ the restatement
def _torch_forward(case, a_mat, a_seq, actions, state_costs, around):
    """an independent float64 statement in torch: tensordot contractions and their diagonals, log-sum-exp by torch, one global beta"""
    f = dc.family(case)
    t = lambda v: torch.as_tensor(np.asarray(v), dtype=torch.float64)
    a_mat, a_seq, acts, costs = t(a_mat), t(a_seq), t(actions), t(state_costs)
    temp = float(f["lam"])
    a_reg = f["lam"] * (1.0 - case["ctrl_penalty"])
    pre = torch.inverse(t(dc.ac.a_cov_of(case)))
    ctrl = a_reg * torch.tensordot(-(acts - a_seq), a_mat @ pre, dims=([-2, -1], [-2, -1]))  # [S, N, N]
    costs = costs + ctrl.diagonal(dim1=-2, dim2=-1)
    eps = acts - (a_mat if around else a_seq)
    log_costs = -(costs - costs.min()) / temp
    eta = log_costs.logsumexp(0)
    omega = (log_costs - eta).exp()
    delta = torch.tensordot(omega.T, eps, dims=1)  # [N, N, H, da]
    new = a_mat + torch.stack([delta[n, n] for n in range(a_mat.shape[0])])
    return dict(costs=costs.numpy(), omega=omega.numpy(), eta=eta.numpy(), a_mix=(eta - eta.logsumexp(0)).exp().numpy(), a_mat=new.numpy())


def _torch_step(case, a_mat, a_mix, strategy, steps, ext):
    f = dc.family(case)
    a_mat = torch.as_tensor(np.array(a_mat), dtype=torch.float64).clone()
    a_mix = torch.as_tensor(np.asarray(a_mix), dtype=torch.float64)
    if strategy == "argmax":
        seq = a_mat[a_mix.argmax()]  # (a view)
    elif strategy == "average":
        seq = torch.einsum("nhd,n->hd", a_mat, a_mix)
    else:
        seq = torch.as_tensor(np.asarray(ext), dtype=torch.float64).clone()
    for i, (lo, hi) in enumerate(zip(f["lo"], f["hi"])):
        seq[..., i].clamp_(lo, hi)
    nxt = seq[:steps].clone()
    seq = seq.roll(-steps, 0)
    seq[-steps:] = 0
    a_mat = a_mat.roll(-steps, 1)
    a_mat[:, -steps:] = 0
    return dict(next=nxt.numpy(), a_seq=seq.numpy(), a_mat=a_mat.numpy())


@pytest.mark.parametrize("cid", dc.IDS)
def test_restatement_against_torch_float64(cid):
    case = dc.BY_ID[cid]
    inp = dc.inputs(case)
    for b in range(case["B"]):
        costs = dc.synthetic_costs(case, b)
        for around in (True, False):
            ours = dc.forward(case, inp["a_mat"][b], inp["a_seq"][b], inp["actions"][b], costs, around)
            ref = _torch_forward(case, inp["a_mat"][b], inp["a_seq"][b], inp["actions"][b], costs, around)
            for k in ref:
                assert elemerr(ours[k], ref[k]) < 1e-12, (cid, b, around, k)
            assert abs(ours["a_mix"].sum() - 1.0) < 1e-12 and np.abs(ours["omega"].sum(0) - 1.0).max() < 1e-12
        for strat in dc.STRATEGIES:
            for steps in sorted({1, case["steps"], case["H"]}):
                ours = dc.step(case, ours_mat := ref["a_mat"], inp["a_seq"][b], ref["a_mix"], strat, steps, inp["ext"][b])
                want = _torch_step(case, ours_mat, ref["a_mix"], strat, steps, inp["ext"][b])
                for k in want:
                    assert np.array_equal(ours[k], want[k]) or elemerr(ours[k], want[k]) < 1e-12, (cid, b, strat, steps, k)
                assert not ours["a_seq"][case["H"] - steps:].any() and not ours["a_mat"][:, case["H"] - steps:].any()


@pytest.mark.parametrize("cid", dc.IDS)
def test_stage_tolerances_and_the_wrong_forms(cid):
    """the tolerances of the stage-wise device check are small, and every wrong form the restatement has lies at least 5 tolerances from
    the right one on the case's own inputs: strategies swapped, control cost dropped, rolled by one instead of `steps`, eps around the
    wrong base, a_mix from unshifted eta, the last maximum instead of the first (the tie)"""
    case = dc.BY_ID[cid]
    tol = dc.stage_tolerance(case)
    assert all(dc.TOL_FLOOR <= v <= 2e-4 for v in tol.values()), tol
    inp = dc.inputs(case)
    N, H = case["N"], case["H"]
    far = {}
    for b in range(case["B"]):
        costs = dc.synthetic_costs(case, b)
        if case["tie"]:
            costs[:, 1] = costs[:, 0]
        args = (inp["a_mat"][b], inp["a_seq"][b], inp["actions"][b], costs)
        fw = dc.forward(case, *args, True)
        st = dc.step(case, fw["a_mat"], inp["a_seq"][b], fw["a_mix"], case["strategy"], case["steps"])

        def keep(name, d):
            far[name] = max(far.get(name, 0.0), d)

        keep("wrong_base", elemerr(dc.forward(case, *args, True, variant="wrong_base")["a_mat"], fw["a_mat"]) / tol["a_mat1"])
        if case["ctrl_penalty"] != 1.0:
            keep("noctrl", elemerr(dc.forward(case, *args, True, variant="noctrl")["omega"], fw["omega"]) / tol["omega"])
        if N > 1 and not case["tie"]:
            keep("unshifted", elemerr(dc.forward(case, *args, True, variant="unshifted")["a_mix"], fw["a_mix"]) / tol["a_mix"])
            keep("swapped", elemerr(dc.step(case, fw["a_mat"], inp["a_seq"][b], fw["a_mix"], case["strategy"], case["steps"], variant="swapped")["next"],
                                    st["next"]) / tol["next"])
        if case["steps"] > 1 and case["steps"] < H:
            keep("roll_one", elemerr(dc.step(case, fw["a_mat"], inp["a_seq"][b], fw["a_mix"], case["strategy"], case["steps"], variant="roll_one")["a_mat"],
                                     st["a_mat"]) / tol["a_mat"])
        if case["tie"]:
            assert fw["a_mix"][0] == fw["a_mix"][1]
            last = dc.step(case, fw["a_mat"], inp["a_seq"][b], fw["a_mix"], "argmax", 1, variant="last_max")
            # (identical rows: the last maximum gives the same sequence, and leaves the clamp on the OTHER row of a_mat)
            assert np.array_equal(last["next"], st["next"])
    print(cid, {k: "%.1e" % v for k, v in tol.items()}, {k: "%.0f" % v for k, v in far.items()})
    for k, v in far.items():
        assert v >= 5.0, (cid, k, v)
    assert "wrong_base" in far


@pytest.mark.parametrize("cid", [c for c in dc.IDS if dc.BY_ID[c]["family"] != "particle" and not dc.BY_ID[c]["nav"] and c != "corner"])
def test_cost_tolerance_and_the_wrong_costs(cid):
    case = dc.BY_ID[cid]
    tol = dc.cost_tolerance(case)
    assert dc.TOL_FLOOR <= tol <= 5e-5, tol
    inp = dc.inputs(case)
    ref = dc.final_costs(case, inp, 0)
    assert np.isfinite(ref).all() and ref.shape == (case["S"], case["N"])
    if case["ctrl_penalty"] != 1.0:
        assert elemerr(dc.final_costs(case, inp, 0, variant="noctrl"), ref) >= 5 * tol
    if case["sigma"]:
        assert elemerr(dc.final_costs(case, inp, 0, uniform_weights=True), ref) >= 5 * tol
        w, scale = dc.sigma_weights(case)
        assert abs(w.sum() - 1.0) < 1e-12 and len(w) == case["M"] == 2 * len(case["up"]) + 1 <= 9 and scale > 0


def test_the_particle_episode_forces_its_events():
    """tests/disco_cases.py EVENTS, from the float64 step alone: environments 0 (crash in period 0), 1 (goal in period 0) and 3 (neither) by
    tests/svmpc_sim_cases.py's proof for the same starts, plant and T; environment 2 is free after period 0 - a position moves by the OLD
    velocity: exact, whatever the action - and on the block after period 1 for every corner of the first action's clamp box"""
    import svmpc_sim_cases as sc
    from oracle import grid_4x4_map

    case, ref, grid = dc.BY_ID["part"], sc.BY_ID["part"], grid_4x4_map()
    st = np.asarray(case["start"], np.float64)
    assert np.array_equal(np.asarray(ref["start"], np.float64), st[[0, 1, 3]]) and ref["T"] == case["T"] and ref["family"] == case["family"]
    r = dc.RULES["part"]
    assert tuple(ref["rules"]["goal"]) == tuple(r["goal"]) and ref["rules"]["radius"] == r["radius"] and ref["rules"]["crash"] and r["crash"]
    assert sc.EVENTS["part"] == {0: dc.EVENTS["part"][0], 1: dc.EVENTS["part"][1]}
    sc.forced_events(ref, grid)  # (asserts its margins)
    f = dc.family(case)
    amax, mass = f["max_accel"], f["defaults"]["mass"]
    corners = np.array([[sx * amax * mass, sy * amax * mass] for sx in (-1, 1) for sy in (-1, 1)] + [[0.0, 0.0]], np.float64) * 3.0
    x1 = dc.ac._step(case, np.repeat(st[2:3], len(corners), 0), corners, dict(f["defaults"]), grid)
    assert not sc.crashed64(ref, x1, grid).any() and sc._frac_margin(grid, x1[:, :2], f["cell"]) >= sc.MARGIN_CELLS
    assert (sc.goal_s64(ref, x1) > r["radius"] ** 2 + sc.MARGIN_S).all()
    for second in corners:  # (the second action cannot move the second position either)
        x2 = dc.ac._step(case, x1, np.repeat(second[None], len(x1), 0), dict(f["defaults"]), grid)
        assert sc.crashed64(ref, x2, grid).all() and sc._frac_margin(grid, x2[:, :2], f["cell"]) >= sc.MARGIN_CELLS


# ------------------------------------------------------------------------------------------------ refusals that need no device
def _ctor(**kw):
    from dust_amd.controllers import BatchDISCO
    from dust_amd.costs import PendulumQuadCos
    from dust_amd.models import PendulumModel

    model, cost = PendulumModel(uncertain_params=("length", "mass")), PendulumQuadCos()
    args = dict(n_envs=3, hz_len=6, n_policies=2, action_samples=16, inst_cost_fn=cost.inst_cost, term_cost_fn=cost.term_cost, params_sampling=None)
    args.update(kw)
    n, H, N, S = (args.pop(k) for k in ("n_envs", "hz_len", "n_policies", "action_samples"))
    return model, BatchDISCO(n, model.observation_space, model.action_space, H, N, S, **args)


def test_the_class_refuses_before_any_device_call():
    """(no device is visible here: a call that reached the library would fail with its own error, not with these)"""
    from dust_amd.models import Particle
    from dust_amd.utils.utf import MerweScaledUTF

    for kw, exc in ((dict(n_envs=0), ValueError), (dict(n_envs=65536), ValueError), (dict(seeds=[1, 2]), ValueError),
                    (dict(n_policies=65), ValueError), (dict(action_samples=1025), ValueError), (dict(hz_len=129), ValueError),
                    (dict(params_sampling=True, params_samples=65), ValueError), (dict(params_sampling="often"), ValueError),
                    (dict(params_sampling=MerweScaledUTF(n=5, alpha=0.5)), ValueError), (dict(inst_cost_fn=None, term_cost_fn=None), ValueError)):
        with pytest.raises(exc):
            _ctor(**kw)
    model, ctrl = _ctor()
    assert tuple(ctrl.a_mat.shape) == (3, 2, 6, 1) and tuple(ctrl.a_seq.shape) == (3, 6, 1) and torch.equal(ctrl.a_mix, torch.ones(3, 2))
    st = torch.zeros(3, 2)
    with pytest.raises(RuntimeError):
        ctrl.step("argmax")
    for call in (lambda: ctrl.step("best"), lambda: ctrl.step("external"), lambda: ctrl.step("average", steps=0), lambda: ctrl.step("average", steps=7),
                 lambda: ctrl.tick(st, model, None, "external"), lambda: ctrl.tick(st, model, None, "average", 7),
                 lambda: ctrl.tick(st, model, None, "average", 1, active=[1, 0]),
                 lambda: ctrl.run_episodes(st, model, None, 0), lambda: ctrl.run_episodes(st, model, None, 4097),
                 lambda: ctrl.run_episodes(st, model, None, 2, "external"), lambda: ctrl.run_episodes(st, model, None, 2, plant_params=torch.ones(3, 2)),
                 lambda: ctrl.simulate(st, model, None, 2, warm_up=1), lambda: ctrl.simulate(st, model, None, 2, goal=[0.0, 0.0]),
                 lambda: ctrl.simulate(st, model, None, 2, goal=[0.0], goal_radius=1.0), lambda: ctrl.simulate(st, model, None, 2, stop_on_crash=True)):
        with pytest.raises(ValueError):
            call()
    assert ctrl._batch is None  # nothing was built
    import copy

    twin = copy.deepcopy(ctrl)
    assert twin._batch is None and torch.equal(twin.a_mat, ctrl.a_mat)


# ------------------------------------------------------------------------------------------------ the reference's closed-loop fixtures
def _fixture(cid):
    return np.load(os.path.join(ROOT, "tests", "golden", "disco_loop_%s.npz" % cid))


@pytest.mark.parametrize("cid", dc.LOOP_IDS)
def test_restatement_reproduces_every_float64_twin(cid):
    """tests/golden/disco_loop_<case>.npz: the restatement of tests/disco_cases.py, chained on itself over the four periods from the
    fixture's inputs, against the float64 run of the reference's own MultiDISCO - forward, step, plant - to 1e-12"""
    case, g = dc.BY_ID[cid], _fixture(cid)
    inp = {k: g[k] for k in ("state", "a_mat0", "a_seq0", "z", "params", "dist_mean", "dist_std", "true") if k in g.files}
    want = dc.loop_inputs(case)
    assert sorted(inp) == sorted(want) and all(np.array_equal(inp[k], want[k]) for k in inp)  # the fixture's inputs are the case's
    assert int(g["T"]) == dc.LOOP_T and str(g["strategy"]) == case["strategy"] and int(g["steps"]) == case["steps"]
    re = dc.restate_loop(case, inp, g["sigma_points"] if case["sigma"] else None)
    for q in dc.LOOP_QUANT:
        assert g[q].dtype == np.float32 and g[q + "_f64"].dtype == np.float64 and g[q].shape == g[q + "_f64"].shape == re[q].shape, q
        assert elemerr(re[q], g[q + "_f64"]) < 1e-12, (cid, q, elemerr(re[q], g[q + "_f64"]))
    chol = np.sqrt(np.diag(dc.ac.a_cov_of(case))).astype(np.float32)
    a_prev = np.concatenate((g["a_mat0"][None], g["a_mat"][:-1]))
    assert elemerr(g["actions"], a_prev[:, None] + chol * g["z"]) < 1e-6  # the recorded actions are a_mat + chol_a z of the period


@pytest.mark.parametrize("cid", dc.LOOP_IDS)
def test_fixture_tolerances_and_off_variants(cid):
    """the stored tolerances are the fp32-to-float64 distance with make_golden_amppi.py's margin (never below 1e-5, never above its cap),
    the fp32 run lies within them, and every `_off` variant the case can show lies at least 5 stored tolerances from the fixture in some
    period (a wrong form need not show in every one: one policy under "average" has a_seq = a_mat from the second period on)"""
    case, g = dc.BY_ID[cid], _fixture(cid)
    T = int(g["T"])
    for q in dc.LOOP_QUANT:
        tol = g["tol_" + q]
        assert tol.shape == (T,) and (tol >= 1e-5).all() and (tol <= 5e-5).all(), (q, tol)
        for k in range(T):
            d = dc.loop_err(g, q, k, g[q][k], g[q + "_f64"][k])
            assert 2.0 * d <= tol[k] * (1 + 1e-6), (cid, q, k, d, tol[k])
    want = sorted("%s_off_%s" % (q, n) for n, (q, shows) in dc.OFF.items() if shows(case))
    assert sorted(k for k in g.files if "_off_" in k) == want
    for name in want:
        q = name.split("_off_")[0]
        far = max(dc.loop_err(g, q, k, g[name][k]) / g["tol_" + q][k] for k in range(T))
        print(cid, name, "%.0f tolerances" % far)
        assert far >= 5.0, (cid, name, far)
    assert {"mppi": 1, "disco": 2, "multi_avg": 5, "multi_arg": 5, "part": 3, "skid": 3, "skid_sigma": 4, "cart": 3}[cid] == len(want)


def test_generator_dry_run_reproduces_the_stored_numbers():
    """where the reference is present: tests/golden/make_golden_disco_loop.py, run dry, gives the stored arrays bit for bit"""
    from oracle import ref_shim

    if not os.path.isdir(os.path.join(ref_shim.REFERENCE_ROOT, "dust")):
        pytest.skip("the reference is not on this machine")
    code = ("import sys; sys.argv = ['x', '--dry']; sys.path.insert(0, 'tests/golden'); import numpy as np; import make_golden_disco_loop as m\n"
            "for cid in m.cases.LOOP_IDS:\n"
            "    g = m.run(m.cases.BY_ID[cid], write=False); s = np.load('tests/golden/disco_loop_%s.npz' % cid)\n"
            "    for k in s.files:\n"
            "        assert np.array_equal(np.asarray(g[k]), s[k]), (cid, k)\n"
            "print('dry run ok')\n")
    out = subprocess.run([os.sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True)
    assert out.returncode == 0 and "dry run ok" in out.stdout, out.stderr[-2000:]
