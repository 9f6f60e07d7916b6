"""The posterior's history without a device: the two entries in the header, the library and the binding; the cap; the six recording
instances and their registers; the Python refusals ahead of any device call; the driver's row assembly on synthetic arrays; the case
table."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import __graft_entry__ as entry
import svmpc_history_cases as cases
from test_svmpc_dual_episode_cpu import _dual
from test_svmpc_dual_sim_cpu import _decl, _kernels

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def built():
    return entry.build()


def test_library_declares_exports_and_binds_the_entries(built):
    from dust_amd import _lib

    VP, I, IP, FP = _lib.VP, C.c_int, C.POINTER(C.c_int), _lib.FP
    lib = C.CDLL(built)
    header = open(os.path.join(ROOT, "include", "dust_amd.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    want = {
        "dust_svmpc_batch_set_history": (["dust_svmpc_batch *batch", "int what"], (I, [VP, I])),
        "dust_svmpc_batch_get_history": (["dust_svmpc_batch *batch", "int which", "int *n_periods", "float *out"], (I, [VP, I, IP, FP])),
    }
    for name, (args, binding) in want.items():
        assert _decl(code, name) == args, name
        assert hasattr(lib, name), name + " is not exported"
        assert _lib.SYMBOLS.get(name) == binding, name
    assert re.search(r"enum\s*\{\s*DUST_HIST_THETA\s*=\s*1\s*,\s*DUST_HIST_FILTER\s*=\s*2\s*\}", code)
    assert (_lib.HIST_THETA, _lib.HIST_FILTER) == (1, 2)
    # the cap: 2^28 floats per kind, in the header and in the binding
    cap = re.search(r"#define\s+DUST_SVMPC_HISTORY_MAX_FLOATS\s+\(\(size_t\)1\s*<<\s*(\d+)\)", code)
    assert cap and int(cap.group(1)) == 28 and _lib.SVMPC_HISTORY_MAX_FLOATS == 1 << 28
    c = cases.CAP
    assert c["T"] * c["B"] * c["N"] * c["H"] * 2 > 1 << 28  # (Particle: da = 2, D = 128) the GPU suite's refusal is one
    # the semantics stand in the header, once
    doc = header[header.index("The posterior's history"):header.index("enum { DUST_HIST_THETA")]
    for words in ("after the t-th per-period call", "dust_mpf_batch_get_particles", "NOT written", "dust_svmpc_batch_set_history(batch, 0) first",
                  "copies the setting, not the recorded rows"):
        assert words in doc, words
    # additive: the version stays
    assert _lib.load().dust_abi_version() == _lib.ABI_VERSION == 3 and "#define DUST_ABI_VERSION 3" in header


def test_the_python_layers_name_the_entries():
    import inspect

    import dust_amd
    import dust_amd.controllers as ctl
    from dust_amd.inference import BatchSVMPC
    from dust_amd.utils import simulations

    sig = inspect.signature(dust_amd.SvmpcBatch.set_history)
    assert list(sig.parameters) == ["self", "theta", "filter"] and all(sig.parameters[k].default is False for k in ("theta", "filter"))
    assert callable(getattr(dust_amd.SvmpcBatch, "history", None))
    for cls in (BatchSVMPC, ctl.BatchDualSVMPC):
        assert callable(getattr(cls, "set_history", None)) and isinstance(getattr(cls, "history", None), property), cls
    # simulate's signatures stand
    sig = inspect.signature(ctl.BatchDualSVMPC.simulate)
    assert list(sig.parameters) == ["self", "states", "n_periods", "goal", "goal_radius", "stop_on_crash", "plant_params", "n_steps", "active", "resume"]
    p = inspect.signature(simulations.run_pendulum_simulations).parameters["history"]
    assert p.kind is inspect.Parameter.KEYWORD_ONLY and p.default is False


def test_exactly_six_recording_instances_without_spill_or_scratch(built, tmp_path):
    """the method of test_svmpc_dual_sim_cpu.py: svmpc_sim_hist_kernel for the four families, svmpc_dual_sim_hist_period_kernel for Pendulum
    and Particle, by name; each without VGPR spill or scratch and within the 256 VGPRs of a 512-lane workgroup"""
    kernels = _kernels(built, tmp_path)
    new = {k: v for k, v in kernels.items() if "hist" in k}
    assert sorted(new) == sorted(cases.HIST_KERNELS), sorted(new)
    for k, (spill, scratch, vgprs) in sorted(new.items()):
        print(k, "spill", spill, "scratch", scratch, "vgprs", vgprs)
        assert spill == 0 and scratch == 0 and vgprs <= 256, (k, spill, scratch, vgprs)
    # no recording kernel hides in the counts the existing tests take by substring
    for old in ("svmpc_sim_kernel", "svmpc_dual_sim_period_kernel", "svmpc_dual_period_kernel", "svmpc_episode_kernel", "svmpc_batch_kernel",
                "svmpc_rows_sim_kernel", "svmpc_skid_nav_sim_kernel"):
        assert not any(old in k for k in new), old


def test_refusals_come_ahead_of_any_device_call():
    import torch

    from dust_amd.models import PendulumModel

    st = torch.zeros(3, 2)
    d, sv, ctrl = _dual(PendulumModel(uncertain_params=("length", "mass")))
    d.set_history(theta=True, filter=True)
    assert sv._history == (True, True) and sv._batch is None  # (kept until a batch is built)
    # per-environment controller rows
    sv._hyper = object()
    with pytest.raises(NotImplementedError, match="per-environment"):
        sv.simulate(st, None, 2)
    sv._hyper = None
    # a navigation cost
    from dust_amd import costs

    real = costs.cost_grid_key
    costs.cost_grid_key = lambda fn: ("a map",)
    try:
        with pytest.raises(NotImplementedError, match="navigation cost"):
            sv.simulate(st, None, 2)
        with pytest.raises(NotImplementedError, match="navigation cost"):
            d.simulate(st, 2)
        sv.set_history(False, True)  # the plain episode records no filter: nothing to refuse - it goes on to its own checks
        with pytest.raises(ValueError, match="n_periods = 0"):
            sv.simulate(st, None, 0)
    finally:
        costs.cost_grid_key = real
    with pytest.raises(RuntimeError, match="nothing is recorded"):
        sv.history
    with pytest.raises(RuntimeError, match="nothing is recorded"):
        d.history
    assert sv._batch is None and ctrl._ctx is None and d._mb is None  # nothing was created: no device call has been made
    assert d._t == 0 and d.ticks == 0 and d._pending is None


def test_deep_copies_carry_the_setting():
    import copy

    from dust_amd.models import PendulumModel

    d, sv, _ = _dual(PendulumModel(uncertain_params=("length", "mass")))
    assert sv._history == (False, False)
    d.set_history(theta=True, filter=False)
    assert copy.deepcopy(sv)._history == (True, False)
    d.set_history(False, False)
    assert copy.deepcopy(sv)._history == (False, False)


# ------------------------------------------------------------------------------------------------ the driver's row assembly
def _synthetic(T_pieces, B=2, N=3, H=2, Mp=4, P=2):
    """theta[t, b, n, h, 0] = 1000 t + 100 b + 10 n + h; x[t, b, m, p] = -(1000 t + 100 b + 10 m + p): t the episode's period"""
    from dust_amd.utils.simulations import posterior_history_columns  # noqa: F401  (the function under test exists)

    steps = sum(T_pieces)
    t, b = np.arange(steps)[:, None, None, None], np.arange(B)[None, :, None, None]
    theta = (1000 * t + 100 * b + 10 * np.arange(N)[None, None, :, None] + np.arange(H)[None, None, None, :]).astype(np.float32)[..., None]
    x = -(1000 * t + 100 * b + 10 * np.arange(Mp)[None, None, :, None] + np.arange(P)[None, None, None, :]).astype(np.float32)
    final = np.full((B, Mp, P), 0.5, np.float32) + np.arange(B, dtype=np.float32)[:, None, None]
    cuts = np.cumsum([0] + list(T_pieces))
    return theta, x, final, [theta[lo:hi] for lo, hi in zip(cuts[:-1], cuts[1:])], [x[lo:hi] for lo, hi in zip(cuts[:-1], cuts[1:])]


@pytest.mark.parametrize("pieces,warm", [((5,), 0), ((5,), 2), ((3, 2), 1), ((2, 3), 4), ((1, 1, 1), 0), ((1,), 0), ((2,), 5)])
def test_row_assembly_follows_the_reference_convention(pieces, warm):
    from dust_amd.utils.simulations import posterior_history_columns

    theta, x, final, th_p, x_p = _synthetic(pieces)
    steps, B = theta.shape[:2]
    dyn, pol = posterior_history_columns(th_p, x_p, final, warm)
    assert dyn.shape == (B, steps) + x.shape[2:] and pol.shape == (B, steps, theta.shape[2])
    assert dyn.dtype == np.float32 and pol.dtype == np.float32
    for b in range(B):
        for t in range(steps):
            # PolParticles: theta[..., 0, 0] after period t; NaN while the episode warms up (simulations.py:122)
            if t < warm:
                assert np.isnan(pol[b, t]).all(), (b, t)
            else:
                assert np.array_equal(pol[b, t], theta[t, b, :, 0, 0]), (b, t)
            # DynParticles: the filter with the pair of period t folded in = recorded row t + 1 - across a piece's end row 0 of the
            # next piece - and at the episode's end the particles that carry the pending update (simulations.py:134-137)
            assert np.array_equal(dyn[b, t], x[t + 1, b] if t + 1 < steps else final[b]), (b, t)
    # the inputs are left as they were
    th2, x2, final2, _, _ = _synthetic(pieces)
    assert np.array_equal(theta, th2) and np.array_equal(x, x2) and np.array_equal(final, final2)


def test_row_assembly_of_environments_that_stopped():
    from dust_amd.utils.simulations import posterior_history_columns

    theta, x, final, th_p, x_p = _synthetic((3, 2), B=3)
    theta, x = theta.copy(), x.copy()
    n_run = np.array([5, 2, 0])
    for b, n in enumerate(n_run):  # what the recording leaves of a row that did not run
        theta[n:, b], x[n:, b] = np.nan, np.nan
    dyn, pol = posterior_history_columns([theta[:3], theta[3:]], [x[:3], x[3:]], final, 1, n_run=n_run)
    assert np.array_equal(dyn[0, :4], x[1:5, 0]) and np.array_equal(dyn[0, 4], final[0])
    assert np.array_equal(dyn[1, 0], x[1, 1]) and np.array_equal(dyn[1, 1], final[1]) and np.isnan(dyn[1, 2:]).all()  # its last pair: pending
    assert np.isnan(dyn[2]).all() and np.isnan(pol[2]).all()
    assert np.isnan(pol[:, 0]).all() and np.array_equal(pol[1, 1], theta[1, 1, :, 0, 0]) and np.isnan(pol[1, 2:]).all()
    with pytest.raises(ValueError):
        posterior_history_columns([theta], [x[:4]], final, 0)
    with pytest.raises(ValueError):
        posterior_history_columns([theta], [x], final[:2], 0)


# ------------------------------------------------------------------------------------------------ the case table
def test_the_case_table_is_the_issues():
    import svmpc_episode_cases as ec

    D = cases.DUAL_BY_ID
    shape = lambda c: (c["N"], c["S"], c["M"], c["H"], c["n_steps"], c["T"], c["B"])
    assert shape(D["P1"]) == (3, 8, 2, 4, 1, 5, 3) and D["P1"]["rules"]["warm_up"] == 2 and (D["P1"]["Mp"], len(D["P1"]["up"])) == (3, 2)
    assert D["P1"]["mpf_bw"] is None and not D["P1"]["first"] and D["P1"]["opts"]["optimizer"] == "SGD" and D["P1"]["opts"]["kernel"] == "K1"
    assert shape(D["P2"])[:6] == (4, 8, 3, 5, 3, 4) and D["P2"]["rules"]["warm_up"] == 1 and D["P2"]["Mp"] == 65 and D["P2"]["log"] and D["P2"]["first"]
    assert D["P2"]["opts"]["optimizer"] == "Adam" and D["P2"]["opts"]["kernel"] == "IMQ"
    assert D["P3"]["family"] == "particle" and D["P3"]["T"] == 4 and (D["P3"]["Mp"], len(D["P3"]["up"])) == (130, 1)
    assert D["P3"]["opts"]["roll_strategy"] == "mean" and D["P3"]["opts"]["weighted_prior"] and D["P3"]["rules"]["crash"]
    assert D["P3"]["start"] == cases.dsc.BY_ID["part_events"]["start"]
    assert shape(D["P4"]) == (1,) * 7 and (D["P4"]["Mp"], len(D["P4"]["up"])) == (1, 1)
    P = cases.PLAIN_BY_ID
    for k, fam in (("P5_skid", "skid"), ("P5_cart", "cartpole")):
        assert P[k]["family"] == fam and shape(P[k])[:6] == (8, 8, 2, 6, 1, 4)
    assert P["P6"]["family"] == "particle" and shape(P["P6"])[:6] == (64, 4, 1, 64, 1, 2) and P["P6"]["H"] * ec.family(P["P6"])["da"] == 128
    # the copy paths: quads and single floats on either side, a row longer than the workgroup's stride, a filter row wider than a wave
    row = lambda c: c["N"] * c["H"] * ec.family(c)["da"]
    xrow = lambda c: c["Mp"] * len(c["up"])
    assert row(D["P1"]) % 4 == 0 and row(D["P7"]) % 4 and row(D["P7"]) > 1 and row(P["P6"]) // 4 > 512
    assert xrow(D["P7"]) % 4 == 0 and xrow(D["P2"]) % 4 and xrow(D["P2"]) > 64 and xrow(D["P3"]) % 4
    assert len(cases.HIST_KERNELS) == 4 + 2
