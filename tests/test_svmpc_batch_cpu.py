"""The batched SVMPC tick without a device: the C ABI's new entries, the register allocation of the four new kernel instances, the
refusals of `BatchSVMPC` that need no device, and the box against the cart-pole tick fixtures."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import __graft_entry__ as entry

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("dust_svmpc_batch_create", "dust_svmpc_batch_destroy", "dust_svmpc_batch_clone", "dust_svmpc_batch_ctx", "dust_svmpc_batch_set",
           "dust_svmpc_batch_get", "dust_svmpc_batch_optimize", "dust_svmpc_batch_forward", "dust_svmpc_batch_tick")


@pytest.fixture(scope="module")
def built():
    return entry.build()


def test_library_declares_exports_and_binds_the_batch_entries(built):
    from dust_amd import _lib

    lib = C.CDLL(built)
    header = open(os.path.join(ROOT, "include", "dust_amd.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    for name in ENTRIES:
        assert re.search(r"\b%s\s*\(" % name, code), name + " is not declared"
        assert hasattr(lib, name), name + " is not exported"
        assert name in _lib.SYMBOLS, name + " is not bound"
    assert "typedef struct dust_svmpc_batch dust_svmpc_batch;" in code
    assert _lib.load().dust_abi_version() == _lib.ABI_VERSION == 3 and "#define DUST_ABI_VERSION 3" in header
    # the flag and the kernel id are appended: nothing that existed moves
    assert "DUST_SVMPC_BATCH_KEEP_ACTIONS = 64" in code and _lib.SVMPC_BATCH_KEEP_ACTIONS == 64
    assert "DUST_K_SVMPC_BATCH = 9" in code and _lib.K_SVMPC_BATCH == 9 and _lib.K_ALL == 10
    assert _lib.load().dust_kernel_name(_lib.K_SVMPC_BATCH) == b"svmpc_batch_kernel"
    for k, name in enumerate(("THETA", "PRIOR_MEANS", "PRIOR_MIX", "A_MAT", "COSTS", "SCORE", "PHI", "LOG_L", "LOG_P", "A_MIX", "ACTIONS")):
        assert "DUST_SVB_%s = %d" % (name, k) in code and getattr(_lib, "SVB_" + name) == k


def test_the_python_layers_name_the_batch():
    import dust_amd
    import dust_amd.inference as inf

    assert hasattr(inf, "BatchSVMPC") and hasattr(dust_amd.Context, "svmpc_batch")
    for m in ("optimize", "forward", "tick", "get", "set", "clone", "close"):
        assert callable(getattr(dust_amd.SvmpcBatch, m)), m
    for m in ("optimize", "forward", "tick", "__deepcopy__"):
        assert callable(getattr(inf.BatchSVMPC, m)), m
    assert isinstance(inf.BatchSVMPC.theta, property) and inf.BatchSVMPC.theta.fset is not None


def test_batch_kernels_do_not_spill(built, tmp_path):
    """the method of test_amppi_batch_cpu.py: the gfx950 code object's metadata shows no VGPR spill and no scratch for the four instances
    of svmpc_batch_kernel"""
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
    mine = {k: v for k, v in kernels.items() if "svmpc_batch_kernel" in k}
    assert len(mine) == 4, sorted(mine)
    for k, (spill, scratch, vgprs) in mine.items():
        assert spill == 0 and scratch == 0 and vgprs <= 256, (k, spill, scratch, vgprs)  # (512 lanes per workgroup: 256 VGPRs per lane)


def _parts(N=4, H=6, S=16, a_cov=None, p_cov=None, **ctrl_kw):
    import torch

    from dust_amd.controllers import MultiDISCO
    from dust_amd.costs import PendulumQuadCos
    from dust_amd.inference import ExponentiatedUtility, get_gmm
    from dust_amd.models import PendulumModel

    model, cost = PendulumModel(), PendulumQuadCos()
    ctrl = MultiDISCO(model.observation_space, model.action_space, H, N, S, a_cov=4.0 * torch.eye(1) if a_cov is None else a_cov,
                      inst_cost_fn=cost.inst_cost, term_cost_fn=cost.term_cost, params_sampling=ctrl_kw.pop("params_sampling", None), **ctrl_kw)
    prior = get_gmm(torch.zeros(N, H, 1), torch.ones(N), 4.0 * torch.eye(1) if p_cov is None else p_cov)
    lik = ExponentiatedUtility(alpha=1.0, n_samples=S, controller=ctrl, model=model)
    return torch.zeros(N, H, 1), prior, lik


def test_constructor_refuses_what_lies_outside_the_box_before_any_device_call():
    import torch

    from dust_amd.inference import BatchSVMPC
    from dust_amd.kernels import IMQ, RBF, RBFKernel, iid_mp
    from dust_amd.utils.utf import MerweScaledUTF

    th, prior, lik = _parts()
    for kernel in (iid_mp(base_kernel=RBF(bandwidth=-1), ctrl_dim=1, indep_controls=True), iid_mp(base_kernel=RBF(), indep_controls=False)):
        with pytest.raises(NotImplementedError, match="K1 .* IMQ"):
            BatchSVMPC(3, th, prior, lik, kernel=kernel)
    with pytest.raises(NotImplementedError, match="resample"):
        BatchSVMPC(3, th, prior, lik, roll_strategy="resample")
    with pytest.raises(ValueError, match="invalid roll strategy"):
        BatchSVMPC(3, th, prior, lik, roll_strategy="shift")
    # a full covariance exists for dim_a = 2: the Particle's action space
    from dust_amd.controllers import MultiDISCO
    from dust_amd.inference import ExponentiatedUtility, get_gmm
    from dust_amd.models import Particle

    pm = Particle(init_state=torch.zeros(4), mass=1.0)
    full = torch.tensor([[1.0, 0.5], [0.5, 1.0]])
    for a_cov, p_cov in ((full, torch.eye(2)), (torch.eye(2), full)):
        ctrl = MultiDISCO(pm.observation_space, pm.action_space, 6, 4, 16, a_cov=a_cov, inst_cost_fn=pm.default_inst_cost,
                          term_cost_fn=pm.default_term_cost, params_sampling=None)
        pr = get_gmm(torch.zeros(4, 6, 2), torch.ones(4), p_cov)
        with pytest.raises(NotImplementedError, match="diagonal covariances"):
            BatchSVMPC(3, torch.zeros(4, 6, 2), pr, ExponentiatedUtility(alpha=1.0, n_samples=16, controller=ctrl, model=pm))
    th_s, prior_s, lik_s = _parts(params_sampling=MerweScaledUTF(n=2))
    with pytest.raises(NotImplementedError, match="sigma-point"):
        BatchSVMPC(3, th_s, prior_s, lik_s)
    th_c, prior_c, lik_c = _parts(ctrl_penalty=0.6)
    with pytest.raises(NotImplementedError, match="ctrl_penalty = 1"):
        BatchSVMPC(3, th_c, prior_c, lik_c)
    th_n, prior_n, lik_n = _parts(N=65)
    with pytest.raises(ValueError, match=r"n_particles = 65 outside \[1, 64\]"):
        BatchSVMPC(3, th_n, prior_n, lik_n)
    for n in (0, 65536):
        with pytest.raises(ValueError, match=r"n_envs = %d outside \[1, 65535\]" % n):
            BatchSVMPC(n, th, prior, lik)
    with pytest.raises(ValueError, match="seeds has 2 entries for 3 environments"):
        BatchSVMPC(3, th, prior, lik, seeds=(1, 2))
    for kernel in (None, RBFKernel(), IMQ(0.7)):  # inside the box: nothing is created yet, theta is the host's
        b = BatchSVMPC(3, th, prior, lik, kernel=kernel, optimizer_class=torch.optim.SGD, lr=0.5, seeds=(7, 7, 9))
        assert b.n_envs == 3 and tuple(b.theta.shape) == (3, 4, 6, 1) and b._batch is None and lik.controller._ctx is None
    b.theta = torch.ones(3, 4, 6, 1)
    assert bool((b.theta == 1).all())
    with pytest.raises(ValueError, match="active has 2 entries"):
        b._active((1, 0))


def test_cartpole_tick_fixtures_lie_inside_the_box():
    from cartpole_cases import TICK_BY_TAG

    for tag in ("tick_k1_sgd", "tick_k1_adam"):
        g = dict(np.load(os.path.join(ROOT, "tests", "golden", "cartpole_%s.npz" % tag), allow_pickle=False))
        s = TICK_BY_TAG[tag]
        K, S, N, H, da = g["eps"].shape
        M, P = g["params"].shape[1:]
        assert (N, S, H, M) == (8, 16, 12, 3) == (s["N"], s["S"], s["H"], s["M"]) and da == 1
        assert 1 <= N <= 64 and 1 <= S <= 1024 and 1 <= M <= 64 and H * da <= 128 and P <= 4
        assert s["kernel"] == "K1" and s.get("ctrl_penalty", 1.0) == 1.0
