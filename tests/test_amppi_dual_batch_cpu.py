"""The batched dual loop without a device: the C ABI's new entries and their signatures, the register allocation of the new kernel
instances, the constructor refusals of `BatchDualAMPPI` and its key schedule."""
import ctypes as C
import os
import re
import shutil
import subprocess

import pytest

import __graft_entry__ as entry

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# entry -> number of parameters in include/dust_amd.h
ENTRIES = dict(dust_mpf_batch_create=3, dust_mpf_batch_destroy=1, dust_mpf_batch_clone=2, dust_mpf_batch_set_particles=2,
               dust_mpf_batch_get_particles=2, dust_mpf_batch_set_obs=2, dust_mpf_batch_get_prior_bw=2, dust_mpf_batch_stats=2,
               dust_mpf_batch_optimize=8, dust_amppi_dual_batch_tick=16)


@pytest.fixture(scope="module")
def built():
    return entry.build()


def test_library_declares_exports_and_binds_the_new_entries(built):
    from dust_amd import _lib

    lib = C.CDLL(built)
    header = open(os.path.join(ROOT, "include", "dust_amd.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    for name, n in ENTRIES.items():
        decl = re.search(r"\b%s\s*\((.*?)\);" % name, code, re.S)
        assert decl, name + " is not declared"
        assert len(decl.group(1).split(",")) == n, (name, decl.group(1))
        assert hasattr(lib, name), name + " is not exported"
        assert name in _lib.SYMBOLS and len(_lib.SYMBOLS[name][1]) == n, name + " is not bound with %d parameters" % n
    assert "typedef struct dust_mpf_batch dust_mpf_batch;" in code
    assert "has no batched form" not in header
    assert _lib.load().dust_abi_version() == _lib.ABI_VERSION == 3 and "#define DUST_ABI_VERSION 3" in header
    tick = re.search(r"int dust_amppi_dual_batch_tick\((.*?)\);", code, re.S).group(1)
    assert "dust_amppi_batch *" in tick and "dust_mpf_batch *" in tick and "const uint64_t *prior_seeds" in tick and "const unsigned char *active" in tick


def test_the_python_layers_name_the_batched_dual_loop():
    import dust_amd
    from dust_amd.controllers import BatchDualAMPPI

    assert callable(dust_amd.MpfContext.batch) and callable(dust_amd.AmppiBatch.dual_tick)
    for m in ("optimize", "set_particles", "get_particles", "set_obs", "get_prior_bw", "stats", "clone", "close"):
        assert callable(getattr(dust_amd.MpfBatch, m)), m
    for m in ("forward", "step", "tick", "prior_keys"):
        assert callable(getattr(BatchDualAMPPI, m)), m
    for p in ("a_seq", "dyn_particles"):
        assert isinstance(getattr(BatchDualAMPPI, p), property), p


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


def test_batched_tick_and_staging_kernels_do_not_spill(built, tmp_path):
    """the method of test_batch_kernels_do_not_spill: no VGPR spill and no scratch for the five instances of the batched tick that draw
    their parameter rows themselves, and for the batched Silverman, sample, sigma-point and heading / angle kernels (two instances)"""
    kernels = _kernels(built, tmp_path)
    mine = {k: v for k, v in kernels.items() if re.search(r"amppi_prior_batch_kernel|amppi_skid_nav_prior_batch_kernel|mpf_silverman_batch_kernel|"
                                                          r"mpf_sample_batch_kernel|mpf_sigma_points_batch_kernel|mpf_lik_angle_batch_kernel", k)}
    assert len(mine) == 10, sorted(mine)
    for k, (spill, scratch, vgprs) in mine.items():
        assert spill == 0 and scratch == 0 and vgprs <= 128, (k, spill, scratch, vgprs)


def test_batched_filter_kernels_do_not_spill(built, tmp_path):
    """no VGPR spill and no scratch for the 44 instances of mpf_optimize_batch_kernel<P, CART, MODEL, LOG, ADAM>: as many particle columns
    as the model has parameters (Pendulum 1 .. 3, Particle 1, skid-steer 1 .. 3, cart-pole 1 .. 4) x parameter space x (Adam, any other
    optimiser).  The body is the lone kernel's text, whose own instances spill (mpf_optimize_kernel<P, false>: 4 / 20 / 38 / 45
    registers at P = 1 .. 4); told their model, its widths, log_space and whether the optimiser is Adam, the batched instances do not."""
    kernels = _kernels(built, tmp_path)
    mine = {k: v for k, v in kernels.items() if "mpf_optimize_batch_kernel" in k}
    assert len(mine) == 44, sorted(mine)
    bad = {k: v for k, v in mine.items() if v[0] != 0 or v[1] != 0 or v[2] > 128}
    assert not bad, "VGPR spills / scratch (name: (spilled VGPRs, scratch bytes, VGPRs)): %r" % bad


def test_lone_filter_kernels_keep_their_registers(built, tmp_path):
    """the lone single-workgroup kernel shares its body text with the batched one (mpf_body.inc): its eight instances keep the spill
    and scratch figures they had before the text moved - (spilled VGPRs, scratch bytes) by (P, CART)"""
    kernels = _kernels(built, tmp_path)
    was = {(1, 1): (0, 0), (1, 0): (4, 20), (2, 1): (0, 0), (2, 0): (20, 84), (3, 1): (0, 0), (3, 0): (38, 156), (4, 1): (7, 32), (4, 0): (45, 184)}
    for (P, cart), (spill, scratch) in was.items():
        name = "_ZN4dust19mpf_optimize_kernelILi%dELb%dEEEvNS_7MpfArgsE" % (P, cart)
        assert name in kernels, name
        assert kernels[name][0] <= spill and kernels[name][1] <= scratch, (name, kernels[name], (spill, scratch))


def _parts(sampling="extended", log_space=False):
    import torch

    from dust_amd.controllers import AMPPI, BatchAMPPI
    from dust_amd.costs import PendulumQuadCos
    from dust_amd.models import PendulumModel

    m, c = PendulumModel(uncertain_params=("length", "mass")), PendulumQuadCos()
    sp = (m.observation_space, m.action_space)
    kw = dict(inst_cost_fn=c.inst_cost, term_cost_fn=c.term_cost, params_sampling=sampling)

    class Dev:
        Mp, P = 8, 2

    class Lik:
        pass

    class Filter:  # what the constructor reads of an MPF: no device behind it
        likelihood, _dev, draw_source, prior = Lik(), Dev(), None, None

    Filter.likelihood.log_space = log_space
    return m, BatchAMPPI(3, *sp, 8, 64, **kw), AMPPI(*sp, 8, 64, **kw), Filter(), torch


def test_constructor_refuses_what_dual_amppi_refuses_and_a_lone_controller():
    from dust_amd.controllers import BatchDualAMPPI
    from dust_amd.utils.utf import MerweScaledUTF

    m, batch, lone, flt, torch = _parts()
    with pytest.raises(TypeError, match="BatchAMPPI"):
        BatchDualAMPPI(lone, m, flt)
    with pytest.raises(ValueError, match="params_sampling='none'"):
        BatchDualAMPPI(_parts(sampling="none")[1], m, flt)
    with pytest.raises(NotImplementedError, match="log-space"):
        BatchDualAMPPI(batch, m, _parts(log_space=True)[3])
    with pytest.raises(ValueError, match="roll=-1"):
        BatchDualAMPPI(batch, m, flt, roll=-1)
    with pytest.raises(NotImplementedError, match="sigma-point transform"):
        BatchDualAMPPI(_parts(sampling=MerweScaledUTF(n=1, alpha=1.0))[1], m, flt)  # a transform over 1 parameter, a filter over 2
    with pytest.raises(ValueError, match="init_particles has shape"):
        BatchDualAMPPI(batch, m, flt, init_particles=torch.zeros(2, 8, 2))
    loop = BatchDualAMPPI(batch, m, flt, init_particles=torch.ones(3, 8, 2), roll=0)
    assert loop.n_envs == 3 and loop.last_bw is None and loop._pending is None and tuple(loop.a_seq.shape) == (3, 8, 1)
    loop.step(torch.zeros(3, 1), torch.zeros(3, 2))  # (noted: nothing reaches a device before forward())
    assert loop._pending is not None and loop._pending[0].shape == (3, 1) and loop._pending[1].shape == (3, 2)


def test_key_schedule():
    """environment b draws under seed + (b << 32) + t in period t = 1, 2, ...: the lone class's seed + t on a per-environment base"""
    from dust_amd.controllers import BatchDualAMPPI

    m, batch, _, flt, _ = _parts()
    loop = BatchDualAMPPI(batch, m, flt, seed=41)
    assert loop.prior_keys(1) == [42, 42 + (1 << 32), 42 + (2 << 32)]
    assert loop.prior_keys(7) == [41 + (b << 32) + 7 for b in range(3)]
    seen = {k for t in range(1, 200) for k in loop.prior_keys(t)}
    assert len(seen) == 3 * 199  # no two (environment, period) pairs meet on one key
    big = BatchDualAMPPI(batch, m, flt, seed=2 ** 64 - 1)
    assert big.prior_keys(1) == [0, 1 << 32, 2 << 32]  # modulo 2^64: what the C ABI's uint64_t holds
