"""The DuSt-MPC loop over a batch of plants without a device: the C ABI's new entry (dust_svmpc_dual_batch_tick), the register allocation
of the four svmpc_prior_batch_kernel instances, the Python layers, the refusals of `BatchDualSVMPC` that need no device, and its key
schedule."""
import ctypes as C
import os
import re
import shutil
import subprocess

import pytest

import __graft_entry__ as entry

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY = "dust_svmpc_dual_batch_tick"


@pytest.fixture(scope="module")
def built():
    return entry.build()


def test_library_declares_exports_and_binds_the_entry(built):
    from dust_amd import _lib

    lib = C.CDLL(built)
    header = open(os.path.join(ROOT, "include", "dust_amd.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    assert hasattr(lib, ENTRY), ENTRY + " is not exported"
    assert ENTRY in _lib.SYMBOLS, ENTRY + " is not bound"
    args = re.search(r"int %s\((.*?)\);" % ENTRY, code, re.S)
    assert args, ENTRY + " is not declared"
    decl = [re.sub(r"\s+", " ", a.strip()) for a in args.group(1).split(",")]
    assert decl == ["dust_svmpc_batch *batch", "dust_mpf_batch *mpf", "const float *states", "const float *actions_prev", "int n_steps",
                    "const void *eps", "int flags", "int mpf_steps", "float mpf_bw", "const uint64_t *prior_seeds",
                    "const unsigned char *active", "float *a_seq", "float *p_weights", "float *params_out", "float *bw_used"], decl
    VP, FP = _lib.VP, _lib.FP
    res, argtypes = _lib.SYMBOLS[ENTRY]
    assert res is C.c_int
    assert argtypes == [VP, VP, FP, FP, C.c_int, VP, C.c_int, C.c_int, C.c_float, C.POINTER(C.c_uint64), C.POINTER(C.c_ubyte), FP, FP, FP, FP]
    # appended: nothing that existed moves
    assert code.index(ENTRY) > code.index("dust_amppi_dual_batch_tick")
    assert _lib.load().dust_abi_version() == _lib.ABI_VERSION == 3 and "#define DUST_ABI_VERSION 3" in header
    assert "DUST_K_SVMPC_BATCH = 9" in code and _lib.K_SVMPC_BATCH == 9 and _lib.K_ALL == 10


def test_the_python_layers_name_the_dual_batch():
    import dust_amd
    import dust_amd.controllers as ctl

    assert callable(dust_amd.SvmpcBatch.dual_tick)
    cls = ctl.BatchDualSVMPC
    for m in ("forward", "step", "tick", "prior_keys", "_flush", "__deepcopy__"):
        assert callable(getattr(cls, m)), m
    for p in ("dyn_particles", "theta"):
        assert isinstance(getattr(cls, p), property), p
    assert "no unfused path" in cls.__doc__ and "warm_up" in cls.__doc__


def test_prior_batch_kernels_do_not_spill(built, tmp_path):
    """the method of test_svmpc_batch_cpu.py test_batch_kernels_do_not_spill on the four instances of svmpc_prior_batch_kernel"""
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
    mine = {k: v for k, v in kernels.items() if "svmpc_prior_batch_kernel" in k}
    assert len(mine) == 4, sorted(mine)
    assert not any("svmpc_batch_kernel" in k for k in mine)  # (the older test counts exactly four names with that substring)
    for k, (spill, scratch, vgprs) in mine.items():
        assert spill == 0 and scratch == 0 and vgprs <= 256, (k, spill, scratch, vgprs)  # (512 lanes per workgroup: 256 VGPRs per lane)


def _parts(N=4, H=6, S=16, sampling=True):
    import torch

    from dust_amd.controllers import MultiDISCO
    from dust_amd.costs import PendulumQuadCos
    from dust_amd.inference import ExponentiatedUtility, get_gmm
    from dust_amd.models import PendulumModel

    model, cost = PendulumModel(uncertain_params=("length", "mass")), PendulumQuadCos()
    ctrl = MultiDISCO(model.observation_space, model.action_space, H, N, S, a_cov=4.0 * torch.eye(1), inst_cost_fn=cost.inst_cost,
                      term_cost_fn=cost.term_cost, params_sampling=True if sampling else None, params_samples=3)
    prior = get_gmm(torch.zeros(N, H, 1), torch.ones(N), 4.0 * torch.eye(1))
    lik = ExponentiatedUtility(alpha=1.0, n_samples=S, controller=ctrl, model=model)
    return torch.zeros(N, H, 1), prior, lik


class _Filter:
    """what the constructor reads of an MPF ahead of any device call"""

    class _Dev:
        Mp, P = 16, 2

    def __init__(self, draw_source=None):
        self.draw_source, self._dev = draw_source, self._Dev()


def test_constructor_refuses_before_any_device_call():
    import torch

    from dust_amd.controllers import BatchDualSVMPC
    from dust_amd.inference import SVMPC, BatchSVMPC

    th, prior, lik = _parts()
    lone = SVMPC(likelihood=lik, init_particles=th, prior=prior, n_particles=4, n_steps=1, optimizer_class=torch.optim.SGD, lr=0.5)
    with pytest.raises(TypeError, match="needs a BatchSVMPC controller, got SVMPC"):
        BatchDualSVMPC(lone, _Filter())
    th0, prior0, lik0 = _parts(sampling=False)
    with pytest.raises(ValueError, match="samples dynamics parameters"):
        BatchDualSVMPC(BatchSVMPC(3, th0, prior0, lik0, optimizer_class=torch.optim.SGD, lr=0.5), _Filter())
    sv = BatchSVMPC(3, th, prior, lik, optimizer_class=torch.optim.SGD, lr=0.5)
    with pytest.raises(NotImplementedError, match="draw_source"):
        BatchDualSVMPC(sv, _Filter(draw_source=object()))
    with pytest.raises(ValueError, match=r"init_particles has shape \(2, 16, 2\), the batch takes \(3, 16, 2\)"):
        BatchDualSVMPC(sv, _Filter(), init_particles=torch.zeros(2, 16, 2))
    loop = BatchDualSVMPC(sv, _Filter(), mpf_steps=7, seed=5, init_particles=torch.ones(3, 16, 2))  # inside: nothing is created yet
    assert loop.n_envs == 3 and loop._mb is None and sv._batch is None and lik.controller._ctx is None and loop.mpf_steps == 7
    assert tuple(loop.theta.shape) == (3, 4, 6, 1) and loop.ticks == 0 and loop.last_bw is None


def test_key_schedule():
    """seed + (b << 32) + t: distinct over B = 256 environments and 1000 periods, and the lone class's `seed + t` on the base
    seed + (b << 32) (DualSVMPC.forward adds one to its seed ahead of every fused call)"""
    import torch

    from dust_amd.controllers import BatchDualSVMPC, DualSVMPC
    from dust_amd.inference import BatchSVMPC

    th, prior, lik = _parts()
    B, T, seed = 256, 1000, 20260
    loop = BatchDualSVMPC(BatchSVMPC(B, th, prior, lik, optimizer_class=torch.optim.SGD, lr=0.5), _Filter(), seed=seed)
    seen = set()
    for t in range(1, T + 1):
        keys = loop.prior_keys(t)
        assert len(keys) == B and all(0 <= k < 1 << 64 for k in keys)
        seen.update(keys)
    assert len(seen) == B * T
    for b in (0, 1, 7, 255):
        lone = DualSVMPC(None, None, fused=True, seed=seed + (b << 32))
        for t in (1, 2, 3, 1000):
            assert loop.prior_keys(t)[b] == lone._seed + t
    top = BatchDualSVMPC(BatchSVMPC(2, th, prior, lik, optimizer_class=torch.optim.SGD, lr=0.5), _Filter(), seed=(1 << 64) - 1)
    assert top.prior_keys(1) == [0, 1 << 32]  # (modulo 2^64)
