"""AMPPI episodes under the reference's rules (dust_amppi_batch_simulate, dust_amppi_dual_batch_simulate; csrc/amppi_episode.hpp
amppi_sim_period_kernel / amppi_skid_nav_sim_period_kernel / amppi_prior_sim_period_kernel) without a device: the C ABI's two entries
and their bindings, the seven new kernel instances and their register allocation, the Python refusals that need no device, and the
power of tests/test_gpu_amppi_sim.py's checks - the forced events, the cost tolerance and its distance from three wrong costs - from the
float64 restatement alone (tests/amppi_sim_cases.py)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import __graft_entry__ as entry
import amppi_sim_cases as cases
from test_amppi_episode_cpu import kernels  # noqa: F401  (the fixture that reads the gfx950 code object's metadata)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def built():
    return entry.build()


def test_library_declares_exports_and_binds_both_entries(built):
    from dust_amd import _lib

    lib = C.CDLL(built)
    header = open(os.path.join(ROOT, "include", "dust_amd.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    FP, UB, IP, RP = _lib.FP, C.POINTER(C.c_ubyte), C.POINTER(C.c_int), C.POINTER(_lib.EpisodeRules)
    want = {
        "dust_amppi_batch_simulate": (C.c_int, [_lib.VP, FP, C.c_int, FP, C.c_int, C.c_int, FP, RP, UB, FP, FP, FP, FP, FP, FP, IP, IP, FP]),
        "dust_amppi_dual_batch_simulate": (C.c_int, [_lib.VP, _lib.VP, FP, FP, C.c_int, C.c_int, C.c_int, C.c_float, C.POINTER(C.c_uint64), C.c_int,
                                                     FP, RP, UB, FP, FP, FP, FP, FP, FP, FP, IP, IP, FP]),
    }
    for name, sig in want.items():
        assert re.search(r"\b%s\s*\(" % name, code), name + " is not declared"
        assert hasattr(lib, name), name + " is not exported"
        assert name in _lib.SYMBOLS, name + " is not bound"
        assert _lib.SYMBOLS[name] == sig, name
    for cite in ("simulations.py:217-260", "124-160", "particle_example.py:191-242"):
        assert cite in header, cite
    assert _lib.load().dust_abi_version() == _lib.ABI_VERSION == 3 and "#define DUST_ABI_VERSION 3" in header
    assert _lib.K_ALL == 10


def test_the_python_layers_name_the_entries():
    import dust_amd
    from dust_amd.controllers import BatchAMPPI, BatchDualAMPPI

    assert callable(getattr(dust_amd.AmppiBatch, "simulate", None)) and callable(getattr(dust_amd.AmppiBatch, "dual_simulate", None))
    assert callable(getattr(BatchAMPPI, "simulate", None)) and callable(getattr(BatchDualAMPPI, "simulate", None))


def test_new_period_kernels_do_not_spill(kernels):  # noqa: F811
    """exactly four family instances, one navigation instance and the Pendulum and Particle prior instances came, each without spilled
    VGPRs or scratch, and none is caught by a substring the existing tests count by"""
    plain = {k: v for k, v in kernels.items() if "amppi_sim_period_kernel" in k}
    nav = {k: v for k, v in kernels.items() if "amppi_skid_nav_sim_period_kernel" in k}
    prior = {k: v for k, v in kernels.items() if "amppi_prior_sim_period_kernel" in k}
    assert len(plain) == 4 and len(nav) == 1 and len(prior) == 2, (sorted(plain), sorted(nav), sorted(prior))
    new = dict(plain, **nav, **prior)
    for k, (vgprs, sgprs, spill, sspill, scratch) in sorted(new.items()):
        print(k, "vgprs", vgprs, "sgprs", sgprs, "spill", spill, "sgpr spill", sspill, "scratch", scratch)
        assert spill == 0 and scratch == 0 and vgprs <= 256, (k, spill, scratch, vgprs)
    for old in ("amppi_period_kernel", "amppi_skid_nav_period_kernel", "amppi_prior_period_kernel", "amppi_kernel", "amppi_batch_kernel",
                "amppi_skid_nav_batch_kernel", "amppi_prior_kernel", "amppi_skid_nav_prior_kernel"):
        assert not any(old in k for k in new), old
    # the period kernels of before and these are the only AMPPI kernels whose name holds `period`
    assert len([k for k in kernels if "amppi" in k and "period" in k]) == 7 + 7


def _part(up=("mass",)):
    import amppi_cases as ac
    from dust_amd.models import Particle

    return Particle(**dict(ac.PART_ENV, mass=2.0, uncertain_params=up))


def _pend(up=("length",)):
    from dust_amd.costs import PendulumQuadCos
    from dust_amd.models import PendulumModel

    return PendulumModel(uncertain_params=up), PendulumQuadCos()


def test_simulate_refuses_before_any_device_call():
    import torch

    from dust_amd.controllers import BatchAMPPI

    m, c = _pend()
    b = BatchAMPPI(3, m.observation_space, m.action_space, 8, 64, inst_cost_fn=c.inst_cost, term_cost_fn=c.term_cost)
    st = torch.zeros(3, 2)
    for T in (0, 4097):
        with pytest.raises(ValueError, match=r"n_periods = %d outside \[1, 4096\]" % T):
            b.simulate(m, st, T)
    with pytest.raises(ValueError, match="steps >= 1"):
        b.simulate(m, st, 2, roll_steps=0)
    with pytest.raises(ValueError, match="active has 2 entries"):
        b.simulate(m, st, 2, active=[1, 0])
    with pytest.raises(ValueError, match="plant_params has shape"):
        b.simulate(m, st, 2, plant_params=torch.ones(2, 1))
    with pytest.raises(ValueError, match="come together"):
        b.simulate(m, st, 2, goal=[0.0, 0.0])
    with pytest.raises(ValueError, match="goal has shape"):
        b.simulate(m, st, 2, goal=[0.0], goal_radius=1.0)
    with pytest.raises(ValueError, match="goal has shape"):
        b.simulate(m, st, 2, goal=[0.0, float("inf")], goal_radius=1.0)
    for r in (0.0, -1.0, float("nan")):
        with pytest.raises(ValueError, match="goal_radius must be finite"):
            b.simulate(m, st, 2, goal=[0.0, 0.0], goal_radius=r)
    with pytest.raises(ValueError, match="stop_on_crash needs an occupancy map"):
        b.simulate(m, st, 2, stop_on_crash=True)

    class Resume:
        t0, loss, status = 2, torch.zeros(2), torch.zeros(2, dtype=torch.int32)

    with pytest.raises(ValueError, match="resume carries 2 environments"):
        b.simulate(m, st, 2, resume=Resume)
    assert b._batch is None  # nothing was created: no device call has been made


def test_dual_simulate_refuses_before_any_device_call():
    import torch

    from dust_amd.controllers import BatchAMPPI, BatchDualAMPPI

    m, c = _pend(("length", "mass"))
    ctrl = BatchAMPPI(3, m.observation_space, m.action_space, 8, 64, inst_cost_fn=c.inst_cost, term_cost_fn=c.term_cost)

    class Filters:
        class _dev:
            P = 2

        class likelihood:
            log_space = False
            model = None

        prior = None

    dual = BatchDualAMPPI.__new__(BatchDualAMPPI)
    dual.controller, dual.model, dual.mpf, dual.roll = ctrl, m, Filters, 1
    dual.n_envs, dual._seed, dual._t, dual._pending, dual.mpf_steps, dual.mpf_bw, dual.ticks, dual.last_bw = 3, 1000, 4, None, 5, None, 4, None
    st = torch.zeros(3, 2)
    for T in (0, 4097):
        with pytest.raises(ValueError, match=r"n_periods = %d outside \[1, 4096\]" % T):
            dual.simulate(st, T)
    with pytest.raises(ValueError, match="plant_params has shape"):
        dual.simulate(st, 2, plant_params=torch.ones(3, 1))
    with pytest.raises(ValueError, match="active has 2 entries"):
        dual.simulate(st, 2, active=[1, 0])
    with pytest.raises(ValueError, match="come together"):
        dual.simulate(st, 2, goal_radius=1.0)
    with pytest.raises(ValueError, match="stop_on_crash needs an occupancy map"):
        dual.simulate(st, 2, stop_on_crash=True)
    dual.roll = 0
    with pytest.raises(ValueError, match="roll >= 1"):
        dual.simulate(st, 2)
    assert ctrl._batch is None and dual._t == 4 and dual.ticks == 4


@pytest.mark.parametrize("cid", sorted(cases.EVENTS))
def test_forced_events_hold_at_every_corner_of_the_action_box(cid):
    case = cases.BY_ID[cid]
    grid = cases.grid_of(case)
    out = cases.forced_events(case, grid)
    print(cid, out)
    assert set(out) == set(range(case["B"]))
    assert sum(1 for b in out if b not in cases.EVENTS[cid]) >= 1  # an environment that no event stops
    for b, (period, status) in cases.EVENTS[cid].items():
        cells, s = out[b]
        assert (cells if status == 2 else s) >= (cases.MARGIN_CELLS if status == 2 else cases.MARGIN_S)


def test_forced_events_of_the_dual_particle_case():
    import amppi_episode_cases as aec

    d = cases.DUAL_BY_ID["part_mass"]
    case = dict(aec._case("dual_part", "particle", d["S"], d["H"], "single", ("mass",), d["T"], 3, 1), rules=d["rules"])
    grid = cases.grid_of(case)
    for rel in (0.6, 1.0, 1.5):  # the true mass is the filters' mean times 0.8 .. 1.25: every row in that range and beyond
        rows = np.full((3, 1), 2.0 * rel, np.float32)
        out = cases.forced_events(case, grid, events=cases.DUAL_EVENTS["part_mass"], start=d["start"], rows=rows)
        assert out[1] == (None, None) and out[0][0] >= cases.MARGIN_CELLS and out[2][0] >= cases.MARGIN_CELLS


@pytest.mark.parametrize("cid", cases.IDS + ["dual_" + d["id"] for d in cases.DUAL])
def test_cost_tolerance_and_power(cid):
    """the tolerance comes from the restatement and stays between floor and cap; each wrong cost the case can show - the previous
    state's, the terminal weights', the one without the obstacle term - lies at least COST_POWER tolerances off in at least one period"""
    case = cases.BY_ID[cid]
    d, tol, power = cases.measure(cid)
    print("%-9s d %.2e tol %.2e  " % (cid, d, tol) + "  ".join("%s %.0f" % kv for kv in sorted(power.items())))
    assert cases.cost_tolerance(case) == tol and cases.TOL_FLOOR <= tol <= cases.TOL_CAP
    want = {"prev_state"} | ({"terminal"} if case["family"] != "pendulum" else set()) | ({"no_obstacle"} if cases.grid_of(case) is not None else set())
    assert set(power) == want
    for k, v in power.items():
        if cases.shows(case, k):
            assert v >= cases.COST_POWER, (cid, k, v)
    assert cases.TOL_FLOOR <= cases.plant_tolerance(case) <= cases.TOL_CAP


def test_the_table_covers_what_the_issue_names():
    by = cases.BY_ID
    assert {by[k]["S"] for k in ("pend257", "part_map", "skid_nav", "cart1021", "one")} == {257, 256, 63, 1021, 1}
    assert by["pend257"]["mode"] == "extended" and by["cart1021"]["mode"] == "single" and by["pend_ut"]["mode"] == "ut"
    assert by["roll3"]["roll_steps"] == 3 and by["skid_nav"]["nav"] and by["skid_nav"]["rules"]["crash"]
    assert by["cart1021"]["rules"]["goal"] is not None and not by["cart1021"]["rules"]["crash"]
    one = by["one"]
    assert one["S"] == one["H"] == one["T"] == one["B"] == 1
    assert sorted(st for _, st in cases.EVENTS["part_map"].values()) == [1, 2, 2] and cases.EVENTS["part_map"][2][0] > 0
    for c in cases.CASES:
        assert c["H"] <= 12 and c["T"] <= 6 and c["B"] <= 5 and c["rules"]["warm_up"] == 0
    d = cases.DUAL_BY_ID
    assert (d["pend_ext"]["Mp"], d["part_mass"]["Mp"], d["pend_sigma"]["Mp"]) == (65, 3, 1)
    assert d["pend_ext"]["bw"] is None and d["pend_ext"]["first"] and d["part_mass"]["bw"] and not d["pend_sigma"]["first"]
    assert {st for _, st in cases.DUAL_EVENTS["part_mass"].values()} == {2} and {p for p, _ in cases.DUAL_EVENTS["part_mass"].values()} == {0, 1}
