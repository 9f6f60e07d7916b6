"""DuSt-MPC episodes on the device (dust_svmpc_dual_batch_episode, csrc/svmpc_episode.hpp svmpc_dual_period_kernel) without a device:
the C ABI's new entry and the Python layers that name it, the register allocation of the two new kernel instances, the refusals of
`BatchDualSVMPC.run_episodes` and `SvmpcBatch.dual_episode` that need no device, the key schedule, and the power of the case table of
tests/svmpc_dual_episode_cases.py - from the float64 restatement alone."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import __graft_entry__ as entry
import svmpc_dual_episode_cases as cases
import svmpc_episode_cases as ec

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def built():
    return entry.build()


def test_library_declares_exports_and_binds_the_entry(built):
    from dust_amd import _lib

    FP, VP, I, U8, U64 = _lib.FP, _lib.VP, C.c_int, C.POINTER(C.c_ubyte), C.POINTER(C.c_uint64)
    lib = C.CDLL(built)
    header = open(os.path.join(ROOT, "include", "dust_amd.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    name = "dust_svmpc_dual_batch_episode"
    decl = re.search(r"\bint\s+%s\s*\((.*?)\)\s*;" % name, code, re.S)
    assert decl, name + " is not declared"
    args = [" ".join(a.split()) for a in decl.group(1).split(",")]
    assert args == ["dust_svmpc_batch *batch", "dust_mpf_batch *mpf", "const float *states", "const float *actions_prev", "int n_periods",
                    "int n_steps", "int mpf_steps", "float mpf_bw", "const uint64_t *prior_seeds", "const float *plant_params", "int flags",
                    "const unsigned char *active", "float *states_out", "float *actions_out", "float *pw_out", "float *bw_out", "float *a_seq"]
    assert hasattr(lib, name), name + " is not exported"
    assert name in _lib.SYMBOLS, name + " is not bound"
    assert _lib.SYMBOLS[name] == (I, [VP, VP, FP, FP, I, I, I, C.c_float, U64, FP, I, U8, FP, FP, FP, FP, FP])
    assert "simulations.py:104-138" in header[header.index("dust_svmpc_dual_batch_episode ="):]
    # additive: the version, the ids and the profile counters stay where they were
    assert _lib.load().dust_abi_version() == _lib.ABI_VERSION == 3 and "#define DUST_ABI_VERSION 3" in header
    assert "DUST_K_SVMPC_BATCH = 9" in code and _lib.K_SVMPC_BATCH == 9 and _lib.K_ALL == 10


def test_the_python_layers_name_the_episode():
    import dust_amd
    import dust_amd.controllers as ctl

    assert callable(getattr(dust_amd.SvmpcBatch, "dual_episode", None))
    assert callable(getattr(ctl.BatchDualSVMPC, "run_episodes", None))


def test_dual_period_kernels_do_not_spill(built, tmp_path):
    """the method of test_svmpc_episode_cpu.py: the gfx950 code object's metadata shows exactly two instances of
    svmpc_dual_period_kernel (Pendulum, Particle), each without VGPR spill or scratch and within 256 VGPRs"""
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
    new = {k: v for k, v in kernels.items() if "svmpc_dual_period_kernel" in k}
    assert len(new) == 2, sorted(new)
    for k, (spill, scratch, vgprs) in new.items():
        print(k, "spill", spill, "scratch", scratch, "vgprs", vgprs)
        assert spill == 0 and scratch == 0 and vgprs <= 256, (k, spill, scratch, vgprs)  # (512 lanes per workgroup: 256 VGPRs per lane)
    # no new kernel hides in the counts the existing tests take by substring
    for old in ("svmpc_episode_kernel", "svmpc_batch_kernel", "svmpc_prior_batch_kernel"):
        assert not any(old in k for k in new), old


class _NoDevice:
    """stands where a device object would: touching it is the failure"""

    def __getattr__(self, name):
        raise AssertionError("a device call (%s) ahead of the refusal" % name)


def _dual(model, B=3, up=("length", "mass")):
    """a BatchDualSVMPC whose controller and filter have made no device object yet"""
    import torch

    from dust_amd.controllers import BatchDualSVMPC, MultiDISCO
    from dust_amd.costs import PendulumQuadCos
    from dust_amd.inference import BatchSVMPC, ExponentiatedUtility, get_gmm

    N, H, S = 3, 6, 16
    cost = PendulumQuadCos()
    ctrl = MultiDISCO(model.observation_space, model.action_space, H, N, S, a_cov=4.0 * torch.eye(1), inst_cost_fn=cost.inst_cost,
                      term_cost_fn=cost.term_cost, params_sampling=True, params_samples=3)
    prior = get_gmm(torch.zeros(N, H, 1), torch.ones(N), 4.0 * torch.eye(1))
    lik = ExponentiatedUtility(alpha=1.0, n_samples=S, controller=ctrl, model=model)
    sv = BatchSVMPC(B, torch.zeros(N, H, 1), prior, lik, optimizer_class=torch.optim.SGD, lr=0.5)

    class _Dev:
        Mp, P = 8, len(up)

    class _Mpf:  # the attributes BatchDualSVMPC reads of an MPF ahead of its first device call
        draw_source, prior, _dev = None, None, _Dev()

        class likelihood:
            pass

    _Mpf.likelihood.model = model
    return BatchDualSVMPC(sv, _Mpf(), mpf_steps=2, seed=40), sv, ctrl


def test_run_episodes_refuses_before_any_device_call():
    import torch

    from dust_amd.models import PendulumModel

    st = torch.zeros(3, 2)
    d, sv, ctrl = _dual(PendulumModel(uncertain_params=("length", "mass")))
    for T in (0, 4097):
        with pytest.raises(ValueError, match=r"n_periods = %d outside \[1, 4096\]" % T):
            d.run_episodes(st, T)
    for bad in (torch.ones(3, 3), torch.ones(2, 2), torch.ones(3)):
        with pytest.raises(ValueError, match="plant_params has shape"):
            d.run_episodes(st, 2, plant_params=bad)
    assert sv._batch is None and ctrl._ctx is None and d._mb is None  # nothing was created: no device call has been made
    assert d._t == 0 and d.ticks == 0 and d._pending is None


@pytest.mark.parametrize("name", ["SkidSteerRobot", "CartPoleModel"])
def test_run_episodes_refuses_the_host_likelihood_families(name):
    import torch

    import dust_amd.models as models

    from dust_amd.models import PendulumModel

    d, sv, ctrl = _dual(PendulumModel(uncertain_params=("length", "mass")))
    cls = getattr(models, name)
    sv.likelihood.model = cls.__new__(cls)  # (the refusal reads the type alone)
    d._pending = (np.zeros((3, 1), np.float32), np.zeros((3, 2), np.float32))
    with pytest.raises(NotImplementedError, match=name):
        d.run_episodes(torch.zeros(3, 2), 2)
    assert sv._batch is None and ctrl._ctx is None and d._mb is None
    assert d._t == 0 and d._pending is not None  # a refused call consumes neither the keys nor the noted update


def test_dual_episode_checks_its_shapes_before_any_device_call():
    from dust_amd import SvmpcBatch

    b = SvmpcBatch.__new__(SvmpcBatch)
    b._h, b.B, b.ds, b.da, b.N, b.H, b.P = _NoDevice(), 3, 2, 1, 4, 5, 2
    mpf = _NoDevice()
    ok = dict(states=np.zeros((3, 2), np.float32), n_periods=2, n_steps=1, seeds=np.zeros((2, 3), np.uint64))
    for bad in (dict(states=np.zeros((2, 2))), dict(states=np.zeros((3, 3))), dict(actions_prev=np.zeros((3, 2))), dict(seeds=np.zeros((3, 2), np.uint64)),
                dict(seeds=np.zeros(6, np.uint64)), dict(seeds=np.zeros((1, 3), np.uint64)), dict(plant_params=np.zeros((3, 3))),
                dict(plant_params=np.zeros((2, 2))), dict(active=[1, 0])):
        with pytest.raises(ValueError):
            b.dual_episode(mpf, **dict(ok, **bad))
    b._h = None  # (nothing to destroy)


def test_key_schedule(monkeypatch):
    """period t of a call made at _t = k draws under prior_keys(k + 1 + t); afterwards _t = k + T and the pair is pending"""
    import torch

    from dust_amd.models import PendulumModel

    d, sv, _ = _dual(PendulumModel(uncertain_params=("length", "mass")))
    B, T, k = 3, 4, 7
    seen = {}

    class _Batch:
        def dual_episode(self, mb, st, n_periods, n_steps, actions_prev, **kw):
            seen.update(kw, T=n_periods, n_steps=n_steps, actions_prev=actions_prev)
            z = np.zeros
            return (np.arange(T * B * 2, dtype=np.float32).reshape(T, B, 2), np.arange(T * B, dtype=np.float32).reshape(T, B, 1), z((T, B, 3), np.float32),
                    np.full((T, B), 0.25, np.float32), z((B, 6, 1), np.float32))

    monkeypatch.setattr(sv, "_ensure_batch", lambda prior: _Batch())
    monkeypatch.setattr(d, "_filters", lambda st=None: object())
    d._t, d.ticks = k, k
    noted = (np.full((B, 1), 0.5, np.float32), np.zeros((B, 2), np.float32))
    d._pending = noted
    xs, acts, pw, a_seq = d.run_episodes(torch.zeros(B, 2), T, n_steps=2)
    assert seen["T"] == T and seen["n_steps"] == 2 and seen["actions_prev"] is noted[0] and seen["mpf_steps"] == 2
    want = np.array([d.prior_keys(k + 1 + t) for t in range(T)], np.uint64)
    assert seen["seeds"].dtype == np.uint64 and np.array_equal(seen["seeds"], want)
    assert want[0, 1] == 40 + (1 << 32) + k + 1 and len({int(v) for v in want.ravel()}) == T * B
    assert d._t == k + T and d.ticks == k + T
    assert np.array_equal(d._pending[0], acts[-1].numpy()) and np.array_equal(d._pending[1], xs[-1].numpy())
    assert np.array_equal(d.last_bw.numpy(), np.full(B, 0.25, np.float32))
    assert tuple(xs.shape) == (T, B, 2) and tuple(acts.shape) == (T, B, 1) and tuple(pw.shape) == (T, B, 3) and tuple(a_seq.shape) == (B, 6, 1)


def _grid(case):
    if case["family"] == "particle":
        from oracle import grid_4x4_map

        return grid_4x4_map()
    return None


@pytest.mark.parametrize("cid", cases.IDS)
def test_power_of_the_case_table(cid):
    """From the restatement alone: under the case's true rows and a deterministic stand-in controller, each wrong plant the case can show
    (nominal parameters, the previous action, no step) lies at least FACTOR tolerances from the right plant in at least one period, and
    the restated loop passes its own check."""
    from helpers import elemerr

    case = cases.BY_ID[cid]
    grid = _grid(case)
    tol = cases.plant_tolerance(case, grid)
    assert ec.TOL_FLOOR <= tol <= ec.TOL_CAP
    xs, acts, exact = cases.restated_loop(case, grid)
    far = cases.variant_distances(case, xs[:-1], acts, exact, tol, grid)
    print("%-22s tol %.2e  " % (cid, tol) + "  ".join("%s %.0f" % kv for kv in sorted(far.items())))
    assert set(far) == ({"nominal", "unstepped"} | ({"prev_action"} if case["T"] > 1 else set()))
    for k, v in far.items():
        assert v >= cases.FACTOR, (cid, k, v)
    assert elemerr(xs[1:], exact) < tol
    # the true rows differ from the nominal ones by 10 - 40 %, another factor per environment
    rel = np.abs(cases.true_rows(case) / ec.nominal_row(case)[None] - 1.0)
    assert (rel >= 0.0999).all() and (rel <= 0.4001).all() and len({tuple(r) for r in np.asarray(case["true_rel"])}) == case["B"]
    assert not np.array_equal(xs[1], xs[0])


def test_the_particle_case_freezes_a_plant():
    """environment 1 of `part_mass_grid` starts on an occupied cell: its state does not move while its neighbours' do"""
    case = cases.BY_ID["part_mass_grid"]
    e = cases.FROZEN["part_mass_grid"]
    xs, _, _ = cases.restated_loop(case, _grid(case))
    assert np.array_equal(xs[:, e], np.broadcast_to(xs[0, e], xs[:, e].shape))
    assert not np.array_equal(xs[1, 0], xs[0, 0]) and not np.array_equal(xs[1, 2], xs[0, 2])
