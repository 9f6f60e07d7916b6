"""DuSt-MPC episodes under the reference's rules (dust_svmpc_dual_batch_simulate, dust_svmpc_dual_batch_optimize, csrc/svmpc_episode.hpp
svmpc_dual_sim_period_kernel) without a device: the C ABI's two new entries and the Python layers that name them, the register allocation
of the two new kernel instances beside the unchanged figures of their neighbours, the refusals that need no device, `warm_up`, the key
schedule of `BatchDualSVMPC.simulate`, and the case table of tests/svmpc_dual_sim_cases.py - from the float64 restatement alone."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import __graft_entry__ as entry
import svmpc_dual_episode_cases as dec
import svmpc_dual_sim_cases as cases
import svmpc_episode_cases as ec
import svmpc_sim_cases as sc
from test_svmpc_dual_episode_cpu import _NoDevice, _dual

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def built():
    return entry.build()


def _decl(code, name):
    decl = re.search(r"\bint\s+%s\s*\((.*?)\)\s*;" % name, code, re.S)
    assert decl, name + " is not declared"
    return [" ".join(a.split()) for a in decl.group(1).split(",")]


def test_library_declares_exports_and_binds_the_entries(built):
    from dust_amd import _lib

    FP, VP, I, U8, U64, IP = _lib.FP, _lib.VP, C.c_int, C.POINTER(C.c_ubyte), C.POINTER(C.c_uint64), C.POINTER(C.c_int)
    lib = C.CDLL(built)
    header = open(os.path.join(ROOT, "include", "dust_amd.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    want = {
        "dust_svmpc_dual_batch_optimize": (
            ["dust_svmpc_batch *batch", "dust_mpf_batch *mpf", "const float *states", "const float *actions_prev", "int n_steps", "const void *eps",
             "int flags", "int mpf_steps", "float mpf_bw", "const uint64_t *prior_seeds", "const unsigned char *active", "float *params_out",
             "float *bw_used"],
            (I, [VP, VP, FP, FP, I, VP, I, I, C.c_float, U64, U8, FP, FP])),
        "dust_svmpc_dual_batch_simulate": (
            ["dust_svmpc_batch *batch", "dust_mpf_batch *mpf", "const float *states", "const float *actions_prev", "int n_periods", "int n_steps",
             "int mpf_steps", "float mpf_bw", "const uint64_t *prior_seeds", "const float *plant_params", "const dust_episode_rules *rules", "int flags",
             "const unsigned char *active", "float *states_out", "float *actions_out", "float *pw_out", "float *bw_out", "float *costs_out", "float *loss",
             "int *status", "int *n_run", "float *a_seq"],
            (I, [VP, VP, FP, FP, I, I, I, C.c_float, U64, FP, C.POINTER(_lib.EpisodeRules), I, U8, FP, FP, FP, FP, FP, FP, IP, IP, FP])),
    }
    for name, (args, binding) in want.items():
        assert _decl(code, name) == args, name
        assert hasattr(lib, name), name + " is not exported"
        assert name in _lib.SYMBOLS, name + " is not bound"
        assert _lib.SYMBOLS[name] == binding, name
    assert "would have left it" in header[header.index("dust_svmpc_dual_batch_simulate ="):]
    assert len(re.findall(r"typedef struct dust_episode_rules", code)) == 1  # the one struct, reused
    # additive: the version, the ids and the profile counters stay where they were
    assert _lib.load().dust_abi_version() == _lib.ABI_VERSION == 3 and "#define DUST_ABI_VERSION 3" in header
    assert "DUST_K_SVMPC_BATCH = 9" in code and _lib.K_SVMPC_BATCH == 9 and _lib.K_ALL == 10


def test_the_python_layers_name_the_entries():
    import inspect

    import dust_amd
    import dust_amd.controllers as ctl
    from dust_amd.utils import simulations

    assert callable(getattr(dust_amd.SvmpcBatch, "dual_optimize", None)) and callable(getattr(dust_amd.SvmpcBatch, "dual_simulate", None))
    assert callable(getattr(ctl.BatchDualSVMPC, "simulate", None))
    sig = inspect.signature(ctl.BatchDualSVMPC.simulate)
    assert list(sig.parameters) == ["self", "states", "n_periods", "goal", "goal_radius", "stop_on_crash", "plant_params", "n_steps", "active", "resume"]
    assert inspect.signature(ctl.BatchDualSVMPC.__init__).parameters["warm_up"].default == 0
    assert callable(getattr(simulations, "run_pendulum_simulations", None))
    assert "mpf" in inspect.signature(simulations.run_particle_episodes).parameters


# the sorted VGPR counts of the instances this change must not move, as the parent commit's build shows them: the four model instances
# of svmpc_prior_batch_kernel and the 44 of mpf_optimize_batch_kernel
PRIOR_VGPRS = [150, 156, 158, 178]
MPF_VGPRS = [77, 77, 80, 80, 83, 84, 84, 87, 87, 87, 93, 95, 95, 95, 96, 98, 99, 99, 102, 103, 105, 109, 109, 110, 110, 111, 111, 114, 116, 118, 119,
             119, 120, 121, 121, 121, 121, 122, 124, 125, 125, 125, 125, 128]


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


def test_dual_sim_period_kernels_do_not_spill_and_the_neighbours_keep_their_registers(built, tmp_path):
    """the method of test_svmpc_dual_episode_cpu.py: exactly two instances of svmpc_dual_sim_period_kernel (Pendulum, Particle), each
    without VGPR spill or scratch and within 256 VGPRs; svmpc_dual_period_kernel, svmpc_prior_batch_kernel and the batched filter
    instances show the figures DESIGN.md section 7 records for them"""
    kernels = _kernels(built, tmp_path)
    new = {k: v for k, v in kernels.items() if "svmpc_dual_sim_period_kernel" in k}
    assert len(new) == 2, sorted(new)
    for k, (spill, scratch, vgprs) in new.items():
        print(k, "spill", spill, "scratch", scratch, "vgprs", vgprs)
        assert spill == 0 and scratch == 0 and vgprs <= 256, (k, spill, scratch, vgprs)  # (512 lanes per workgroup: 256 VGPRs per lane)
    for old in ("svmpc_dual_period_kernel", "svmpc_sim_kernel", "svmpc_episode_kernel", "svmpc_batch_kernel", "svmpc_prior_batch_kernel"):
        assert not any(old in k for k in new), old  # no new kernel hides in the counts the existing tests take by substring
    period = sorted(v for k, v in kernels.items() if "svmpc_dual_period_kernel" in k)
    assert period == [(0, 0, 153), (0, 0, 160)], period
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    for name in ("svmpc_prior_batch_kernel", "mpf_optimize_batch_kernel"):
        inst = {k: v for k, v in kernels.items() if name in k and "nav" not in k}
        assert inst and all(v[0] == 0 and v[1] == 0 for v in inst.values()), name
    prior = sorted(v[2] for k, v in kernels.items() if "svmpc_prior_batch_kernel" in k and "nav" not in k)
    assert prior == PRIOR_VGPRS, prior
    mpf = sorted(v[2] for k, v in kernels.items() if "mpf_optimize_batch_kernel" in k)
    assert mpf == MPF_VGPRS, mpf
    for k, (_, _, vgprs) in new.items():
        assert "%d" % vgprs in design[design.index("the two instances of `svmpc_dual_sim_period_kernel` take"):][:120], (k, vgprs)


def test_refusals_come_ahead_of_any_device_call():
    import torch

    from dust_amd.models import PendulumModel

    st = torch.zeros(3, 2)
    d, sv, ctrl = _dual(PendulumModel(uncertain_params=("length", "mass")))
    for T in (0, 4097):
        with pytest.raises(ValueError, match=r"n_periods = %d outside \[1, 4096\]" % T):
            d.simulate(st, T)
    for bad in (torch.ones(3, 3), torch.ones(2, 2), torch.ones(3)):
        with pytest.raises(ValueError, match="plant_params has shape"):
            d.simulate(st, 2, plant_params=bad)
    with pytest.raises(ValueError, match="come together"):
        d.simulate(st, 2, goal=(0.0, 0.0))
    with pytest.raises(ValueError, match="goal has shape"):
        d.simulate(st, 2, goal=(0.0, 0.0, 0.0), goal_radius=1.0)
    with pytest.raises(ValueError, match="goal has shape"):
        d.simulate(st, 2, goal=(0.0, float("nan")), goal_radius=1.0)
    for r in (0.0, -1.0, float("inf")):
        with pytest.raises(ValueError, match="goal_radius"):
            d.simulate(st, 2, goal=(0.0, 0.0), goal_radius=r)
    with pytest.raises(ValueError, match="stop_on_crash needs an occupancy map"):
        d.simulate(st, 2, stop_on_crash=True)
    sv._hyper = object()
    with pytest.raises(NotImplementedError, match="per-environment"):
        d.simulate(st, 2)
    sv._hyper = None
    assert sv._batch is None and ctrl._ctx is None and d._mb is None  # nothing was created: no device call has been made
    assert d._t == 0 and d.ticks == 0 and d._pending is None


@pytest.mark.parametrize("name", ["SkidSteerRobot", "CartPoleModel"])
def test_simulate_refuses_the_host_likelihood_families(name):
    import torch

    import dust_amd.models as models
    from dust_amd.models import PendulumModel

    d, sv, ctrl = _dual(PendulumModel(uncertain_params=("length", "mass")))
    cls = getattr(models, name)
    sv.likelihood.model = cls.__new__(cls)  # (the refusal reads the type alone)
    d._pending = (np.zeros((3, 1), np.float32), np.zeros((3, 2), np.float32))
    with pytest.raises(NotImplementedError, match=name):
        d.simulate(torch.zeros(3, 2), 2)
    assert sv._batch is None and ctrl._ctx is None and d._mb is None
    assert d._t == 0 and d._pending is not None  # a refused call consumes neither the keys nor the noted update


def test_the_bindings_check_their_shapes_before_any_device_call():
    from dust_amd import SvmpcBatch

    b = SvmpcBatch.__new__(SvmpcBatch)
    b._h, b.B, b.ds, b.da, b.N, b.H, b.P, b.M = _NoDevice(), 3, 2, 1, 4, 5, 2, 2
    mpf = _NoDevice()
    ok = dict(states=np.zeros((3, 2), np.float32), n_periods=2, n_steps=1, seeds=np.zeros((2, 3), np.uint64))
    for bad in (dict(states=np.zeros((2, 2))), dict(states=np.zeros((3, 3))), dict(actions_prev=np.zeros((3, 2))), dict(seeds=np.zeros((3, 2), np.uint64)),
                dict(seeds=np.zeros(6, np.uint64)), dict(seeds=np.zeros((1, 3), np.uint64)), dict(plant_params=np.zeros((3, 3))),
                dict(plant_params=np.zeros((2, 2))), dict(active=[1, 0]), dict(goal=(0.0, 0.0, 0.0), goal_radius=1.0), dict(loss=np.zeros(2)),
                dict(status=np.zeros(4, np.int32))):
        with pytest.raises(ValueError):
            b.dual_simulate(mpf, **dict(ok, **bad))
    for bad in (dict(states=np.zeros((2, 2))), dict(actions_prev=np.zeros((3, 2))), dict(active=[1, 0])):
        with pytest.raises(ValueError):
            b.dual_optimize(mpf, **dict(dict(states=np.zeros((3, 2), np.float32), n_steps=1, seeds=np.zeros(3, np.uint64)), **bad))
    b._h = None  # (nothing to destroy)


def test_warm_up_constructs_and_defaults_to_zero():
    from dust_amd.controllers import BatchDualSVMPC
    from dust_amd.models import PendulumModel

    d, sv, _ = _dual(PendulumModel(uncertain_params=("length", "mass")))
    assert d.warm_up == 0
    w = BatchDualSVMPC(sv, d.mpf, mpf_steps=2, seed=40, warm_up=3)
    assert w.warm_up == 3 and w.ticks == 0
    with pytest.raises(ValueError, match="warm_up"):
        BatchDualSVMPC(sv, d.mpf, warm_up=-1)


def test_key_schedule_of_simulate(monkeypatch):
    """period t of a call made at _t = k draws under prior_keys(k + 1 + t); the period index starts at resume.t0; environments with
    resume.status != 0 are passed as inactive; afterwards _t = k + T and the noted update is (actions[n_run - 1], states[n_run - 1]) per
    environment, or the pair it came with when n_run <= 0; a refused call consumes neither"""
    import torch

    from dust_amd.controllers.dual import DualSimResult
    from dust_amd.models import PendulumModel

    d, sv, _ = _dual(PendulumModel(uncertain_params=("length", "mass")))
    d.warm_up = 5
    B, T, k = 3, 4, 7
    seen = {}
    n_run = np.array([4, 2, 0], np.int32)
    xs = np.arange(T * B * 2, dtype=np.float32).reshape(T, B, 2)
    acts = np.arange(T * B, dtype=np.float32).reshape(T, B, 1) + 100

    class _Batch:
        H, da = 6, 1

        def dual_simulate(self, mb, st, n_periods, n_steps, actions_prev, **kw):
            seen.update(kw, T=n_periods, n_steps=n_steps, actions_prev=actions_prev)
            if kw["plant_params"] is not None:
                raise RuntimeError("refused")
            z = np.zeros
            return (xs, acts, z((T, B, 3), np.float32), np.full((T, B), 0.25, np.float32), z((T, B), np.float32), z(B, np.float32),
                    np.array([0, 1, 2], np.int32), n_run, z((B, 6, 1), np.float32))

    monkeypatch.setattr(sv, "_ensure_batch", lambda prior: _Batch())
    monkeypatch.setattr(d, "_filters", lambda st=None: object())
    d._t, d.ticks = k, k
    noted = (np.full((B, 1), 0.5, np.float32), np.full((B, 2), -1.0, np.float32))
    d._pending = noted
    resume = DualSimResult(*([None] * 5), torch.zeros(B), torch.tensor([0, 0, 2], dtype=torch.int32), None, None)
    resume.t0 = 3
    start = torch.full((B, 2), 9.0)
    with pytest.raises(RuntimeError, match="refused"):
        d.simulate(start, T, plant_params=np.ones((B, 2), np.float32), resume=resume)
    assert d._t == k and d.ticks == k and d._pending is noted
    res = d.simulate(start, T, n_steps=2, resume=resume)
    assert seen["T"] == T and seen["n_steps"] == 2 and seen["actions_prev"] is noted[0] and seen["mpf_steps"] == 2
    assert seen["t0"] == 3 and seen["warm_up"] == 5 and list(seen["active"]) == [True, True, False]
    want = np.array([d.prior_keys(k + 1 + t) for t in range(T)], np.uint64)
    assert seen["seeds"].dtype == np.uint64 and np.array_equal(seen["seeds"], want)
    assert want[0, 1] == 40 + (1 << 32) + k + 1 and len({int(v) for v in want.ravel()}) == T * B
    assert d._t == k + T and d.ticks == k + T and res.t0 == 3 + T
    assert np.array_equal(d._pending[0], np.stack([acts[3, 0], acts[1, 1], noted[0][2]]))
    assert np.array_equal(d._pending[1], np.stack([xs[3, 0], xs[1, 1], start[2].numpy()]))
    assert res._fields == ("states", "actions", "p_weights", "bw", "costs", "loss", "status", "n_run", "a_seq")


def test_forward_while_warming_up_calls_dual_optimize(monkeypatch):
    """ticks < warm_up: forward() is dust_svmpc_dual_batch_optimize, a zero a_seq [B, H, da] and None for the weights"""
    import torch

    from dust_amd.models import PendulumModel

    d, sv, _ = _dual(PendulumModel(uncertain_params=("length", "mass")))
    d.warm_up = 2
    calls = []

    class _Batch:
        H, da = 6, 1

        def dual_optimize(self, mb, st, ap, **kw):
            calls.append(("optimize", kw["seeds"]))
            return None, np.zeros(3, np.float32)

        def dual_tick(self, mb, st, ap, **kw):
            calls.append(("tick", kw["seeds"]))
            return np.ones((3, 6, 1), np.float32), np.ones((3, 3), np.float32), None, np.zeros(3, np.float32)

    monkeypatch.setattr(sv, "_ensure_batch", lambda prior: _Batch())
    monkeypatch.setattr(d, "_filters", lambda st=None: object())
    monkeypatch.setattr("dust_amd.inference.svmpc.check_optimizer", lambda *a: None)
    for t in range(3):
        a_seq, pw = d.forward(torch.zeros(3, 2))
        if t < 2:
            assert pw is None and tuple(a_seq.shape) == (3, 6, 1) and not a_seq.any()
        else:
            assert pw is not None and a_seq.all()
        d.step(a_seq[:, 0], torch.zeros(3, 2))
    assert [c[0] for c in calls] == ["optimize", "optimize", "tick"] and [c[1] for c in calls] == [d.prior_keys(t) for t in (1, 2, 3)]


# ------------------------------------------------------------------------------------------------ the case table, from float64 alone
def test_the_case_table_is_the_issues():
    c = cases.BY_ID
    assert cases.IDS == ["pend_warm", "pend_adam_first", "pend_log", "part_events", "part_warm_events", "ones"]
    key = lambda x: tuple(x[k] for k in ("N", "S", "M", "H", "n_steps", "T", "B"))
    assert key(c["pend_warm"]) == (3, 8, 3, 5, 1, 5, 3) and c["pend_warm"]["rules"]["warm_up"] == 2 and c["pend_warm"]["mpf_bw"] is None
    assert c["pend_warm"]["opts"]["optimizer"] == c["pend_warm"]["filt_opt"] == "SGD"
    a = c["pend_adam_first"]
    assert key(a) == (4, 16, 8, 6, 3, 4, 2) and a["opts"]["kernel"] == "IMQ" and a["opts"]["optimizer"] == a["filt_opt"] == "Adam"
    assert a["Mp"] == 65 and a["mpf_bw"] == 0.3 and a["first"] and a["rules"]["warm_up"] == 1
    lg = c["pend_log"]
    assert lg["log"] and lg["Mp"] == 3 and lg["T"] == 3 and lg["B"] == 2 and lg["rules"]["warm_up"] == 0
    pe, pw = c["part_events"], c["part_warm_events"]
    assert pe["family"] == pw["family"] == "particle" and pe["up"] == pw["up"] == ("mass",) and pe["B"] == pw["B"] == 4
    assert pe["rules"]["warm_up"] == 0 and pw["rules"]["warm_up"] == 3 and pw["T"] == 4
    assert key(c["ones"]) == (1, 1, 1, 1, 1, 1, 1) and c["ones"]["Mp"] == 1 and c["ones"]["mpf_steps"] == 1 and cases.WARM_TOO == {"ones": 1}
    for case in cases.CASES:  # the true rows differ from the nominal ones by 10 - 40 %, another factor per environment
        rel = np.abs(dec.true_rows(case) / ec.nominal_row(case)[None] - 1.0)
        assert (rel >= 0.0999).all() and (rel <= 0.4001).all() and len({tuple(r) for r in np.asarray(case["true_rel"])}) == case["B"]


@pytest.mark.parametrize("cid", sorted(cases.EVENTS))
def test_forced_events_hold_under_the_true_rows(cid):
    """part_events: for every action inside the clamps; part_warm_events: under the zero action; with svmpc_sim_cases' margins, and the
    fp32 replicas agree with the float64 predicates at those states (asserted inside forced_events)"""
    case = cases.BY_ID[cid]
    grid = cases.grid_of(case)
    got = cases.forced_events(case, grid)
    print(cid, got)
    for b, (period, status) in cases.EVENTS[cid].items():
        cells, s = got[b]
        assert (cells is not None and cells >= sc.MARGIN_CELLS) if status == 2 else (s is not None and s >= sc.MARGIN_S)
    assert all(got[b] == (None, None) for b in range(case["B"]) if b not in cases.EVENTS[cid])
    if cid == "part_events":  # environment 0 starts ON an occupied cell
        assert sc.crashed64(case, ec.start_states(case)[:1].astype(np.float64), grid)[0]
    else:  # neighbours stop in different periods
        n, st = cases.expected(case)
        assert list(n) == [2, 2, 3, 4] and list(st) == [2, 1, 1, 0]
    xs, _, _, n_run, status = cases.restated_loop(case, grid)
    n, st = cases.expected(case)
    assert np.array_equal(n_run, n) and np.array_equal(status, st)


@pytest.mark.parametrize("cid", cases.IDS)
def test_power_of_the_case_table(cid):
    """Under the stand-in controller: at least one period's cost lies COST_FACTOR tolerances from each wrong cost the case can show, the
    plant keeps the dual-episode cases' FACTOR from its three wrong plants, and the restated loop passes its own checks"""
    from helpers import elemerr

    for warm in [None] + ([cases.WARM_TOO[cid]] if cid in cases.WARM_TOO else []):
        case = cases.BY_ID[cid] if warm is None else cases.with_rules(cases.BY_ID[cid], warm_up=warm)
        grid = cases.grid_of(case)
        tol = cases.cost_tolerance(case)
        assert tol == sc.cost_tolerance(sc.BY_ID["pend" if case["family"] == "pendulum" else "part"]) and sc.TOL_FLOOR <= tol <= sc.TOL_CAP
        xs, acts, exact, n_run, status = cases.restated_loop(case, grid)
        far = cases.cost_power(case, xs, n_run, grid, tol)
        print("%-18s cost tol %.2e  " % (cid, tol) + "  ".join("%s %.0f" % kv for kv in sorted(far.items())))
        assert set(far) == cases.cost_variants_shown(case)
        for k, v in far.items():
            assert v >= cases.COST_FACTOR, (cid, k, v)
        ptol = dec.plant_tolerance(case, grid)
        pfar = dec.variant_distances(case, xs[:-1], acts, exact, ptol, grid)
        print("%-18s plant tol %.2e  " % (cid, ptol) + "  ".join("%s %.0f" % kv for kv in sorted(pfar.items())))
        assert set(pfar) == ({"nominal", "unstepped"} | ({"prev_action"} if case["T"] > 1 else set()))
        for k, v in pfar.items():
            assert v >= cases.FACTOR, (cid, k, v)
        assert elemerr(xs[1:], exact) < ptol
        assert not acts[:case["rules"]["warm_up"]].any()
