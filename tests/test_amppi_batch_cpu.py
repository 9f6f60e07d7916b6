"""The batched AMPPI tick without a device: the C ABI's new entries, the register allocation of the five new kernel instances and the
refusals of `BatchAMPPI` that need no device."""
import ctypes as C
import os
import re
import shutil
import subprocess

import pytest

import __graft_entry__ as entry

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("dust_amppi_batch_create", "dust_amppi_batch_destroy", "dust_amppi_batch_clone", "dust_amppi_batch_set_a_seq",
           "dust_amppi_batch_get_a_seq", "dust_amppi_batch_update", "dust_amppi_batch_roll", "dust_amppi_batch_get_actions",
           "dust_amppi_batch_ctx")


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
    assert "typedef struct dust_amppi_batch dust_amppi_batch;" in code
    assert _lib.load().dust_abi_version() == _lib.ABI_VERSION == 3 and "#define DUST_ABI_VERSION 3" in header


def test_the_python_layers_name_the_batch():
    import dust_amd
    from dust_amd.controllers import AMPPI, BatchAMPPI

    assert issubclass(BatchAMPPI, AMPPI) and hasattr(dust_amd.Context, "amppi_batch")
    for m in ("update", "roll", "get_a_seq", "set_a_seq", "clone", "close"):
        assert callable(getattr(dust_amd.AmppiBatch, m)), m


def test_batch_kernels_do_not_spill(built, tmp_path):
    """the method of test_amppi_kernels_do_not_spill: the gfx950 code object's metadata shows no VGPR spill and no scratch for the four
    instances of amppi_batch_kernel and for amppi_skid_nav_batch_kernel"""
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
    mine = {k: v for k, v in kernels.items() if "amppi_batch_kernel" in k or "amppi_skid_nav_batch_kernel" in k}
    assert len(mine) == 5, sorted(mine)
    for k, (spill, scratch, vgprs) in mine.items():
        assert spill == 0 and scratch == 0 and vgprs <= 128, (k, spill, scratch, vgprs)


def _pend():
    from dust_amd.costs import PendulumQuadCos
    from dust_amd.models import PendulumModel

    return PendulumModel(uncertain_params=("length",)), PendulumQuadCos()


def test_constructor_refuses_what_amppi_refuses():
    import torch

    from dust_amd.controllers import BatchAMPPI

    m, c = _pend()
    sp = (m.observation_space, m.action_space)
    kw = dict(inst_cost_fn=c.inst_cost, term_cost_fn=c.term_cost)
    with pytest.raises(ValueError, match="Invalid value for 'params_sampling': all"):
        BatchAMPPI(3, *sp, 8, 64, params_sampling="all", **kw)
    with pytest.raises(ValueError, match="Specify at least one cost function"):
        BatchAMPPI(3, *sp, 8, 64)
    with pytest.raises(NotImplementedError, match="dim_a = 2"):
        BatchAMPPI(3, *sp, 8, 64, a_cov=torch.tensor([[1.0, 0.5], [0.5, 1.0]]), **kw)
    for n in (0, 65536):
        with pytest.raises(ValueError, match=r"n_envs = %d outside \[1, 65535\]" % n):
            BatchAMPPI(n, *sp, 8, 64, **kw)
    with pytest.raises(ValueError, match="seeds has 2 entries for 3 environments"):
        BatchAMPPI(3, *sp, 8, 64, seeds=(1, 2), **kw)
    init = torch.arange(8.0).view(8, 1)
    b = BatchAMPPI(3, *sp, 8, 64, init_actions=init, seeds=(7, 7, 9), **kw)
    assert b.n_envs == 3 and tuple(b.a_seq.shape) == (3, 8, 1) and all(torch.equal(b.a_seq[k], init) for k in range(3))
    b.roll(3, active=(1, 0, 1))  # before any device context: on the host
    assert torch.equal(b.a_seq[1], init) and torch.equal(b.a_seq[0, :5], init[3:]) and not b.a_seq[2, 5:].any()
    with pytest.raises(ValueError):
        b.roll(0)
    with pytest.raises(ValueError, match="active has 2 entries"):
        b.roll(1, active=(1, 0))


def test_config_refuses_what_amppi_refuses_before_any_device_call():
    import torch

    import amppi_cases as cases
    from dust_amd.controllers import BatchAMPPI
    from dust_amd.costs import QuadraticCost
    from dust_amd.models import CartPoleModel, Particle

    m, c = _pend()
    sp = (m.observation_space, m.action_space)
    kw = dict(inst_cost_fn=c.inst_cost, term_cost_fn=c.term_cost)
    states = torch.tensor([[3.0, 0.0]] * 2)

    class Other:
        family = "walker"

    with pytest.raises(NotImplementedError, match="no AMPPI kernel family"):
        BatchAMPPI(2, *sp, 8, 64, **kw).update_actions(Other(), states)
    with pytest.raises(NotImplementedError, match="128"):
        BatchAMPPI(2, *sp, 129, 64, params_sampling="none", **kw).update_actions(m, states)
    with pytest.raises(NotImplementedError, match="65536"):
        BatchAMPPI(2, *sp, 8, 65537, params_sampling="none", **kw).update_actions(m, states)
    cart = CartPoleModel()
    qc = QuadraticCost((0, 0, 0, 0), (1, 1, 1, 1), w_ctrl=(0.1,))
    with pytest.raises(NotImplementedError, match="w_ctrl"):
        BatchAMPPI(2, cart.observation_space, cart.action_space, 8, 64, inst_cost_fn=qc.inst_cost, term_cost_fn=qc.term_cost,
                   params_sampling="none").update_actions(cart, torch.zeros(2, 4))
    q0 = QuadraticCost((0, 0, 0, 0), (1, 1, 1, 1))
    with pytest.raises(ValueError, match="uncertain_params"):
        BatchAMPPI(2, cart.observation_space, cart.action_space, 8, 64, inst_cost_fn=q0.inst_cost, term_cost_fn=q0.term_cost).update_actions(cart, torch.zeros(2, 4))
    noisy = Particle(**dict(cases.PART_ENV, deterministic=False), mass=2.0)
    with pytest.raises(NotImplementedError, match="deterministic"):
        BatchAMPPI(2, noisy.observation_space, noisy.action_space, 8, 64, inst_cost_fn=noisy.default_inst_cost,
                   term_cost_fn=noisy.default_term_cost, params_sampling="none").update_actions(noisy, torch.zeros(2, 4))
