"""The cart-pole family without a GPU: the library exports and binds its two entries and the struct sizes agree, the host
`CartPoleModel.step` is the reference's bit for bit, a float64 numpy restatement of the closed-form parameter Jacobian (the forms
mpf.hpp's mpf_cart_score evaluates, written out again below) reproduces the reference's float64 autograd, the fixtures of
tests/golden/make_golden_cartpole.py / make_golden_mpf_cartpole.py keep their caps and their power, the rollout kernel compiles without
spills or scratch, and the host layer accepts and refuses what it should."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

import __graft_entry__ as entry
from cartpole_cases import (BY_TAG, NAMES, NAMES7, ROLLOUT_BY_TAG, ROLLOUT_NAMES, ROLLOUT_QUANT, SWEEP_SIZES, TICK_NAMES, TICK_QUANT, lead_quantity,
                            particles, sweep_scenario, twin)
from helpers import elemerr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CAP, CAP_DISP, TOL = 5e-5, 2e-3, 1e-5
QUANT = ("phi0", "x_2", "grad_norms_2", "x_n", "grad_norms", "x_n2", "grad_norms2", "probe_log_prob")


@pytest.fixture(scope="module")
def built():
    return entry.build()


# ---------------------------------------------------------------------------------------------- the C ABI
def test_library_exports_and_binds_the_cartpole_entries(built, tmp_path):
    from dust_amd import _lib

    lib = C.CDLL(built)
    for name in ("dust_set_cartpole", "dust_mpf_set_cartpole"):
        assert hasattr(lib, name) and name in _lib.SYMBOLS
    assert _lib.SYMBOLS["dust_mpf_set_cartpole"] == _lib.SYMBOLS["dust_set_cartpole"]  # (handle, const dust_cartpole_config *)
    assert _lib.MODEL_CARTPOLE == 3
    # sizeof / offsets of dust_cartpole_config as a C compiler lays the header's struct out
    cc = shutil.which("gcc") or shutil.which("cc")
    assert cc, "no C compiler"
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "dust_amd.h"\nint main(void) { printf("%zu %zu %zu %zu %d\\n", '
                   'sizeof(dust_cartpole_config), offsetof(dust_cartpole_config, mu_p), offsetof(dust_cartpole_config, goal), '
                   'offsetof(dust_cartpole_config, w_ctrl), (int)DUST_MODEL_CARTPOLE); return 0; }\n')
    exe = str(tmp_path / "sz")
    subprocess.run([cc, "-I" + os.path.join(ROOT, "include"), str(src), "-o", exe], check=True)
    size, o_mup, o_goal, o_wc, model = (int(v) for v in subprocess.run([exe], check=True, capture_output=True, text=True).stdout.split())
    T = _lib.CartPoleConfig
    assert (size, o_mup, o_goal, o_wc, model) == (C.sizeof(T), T.mu_p.offset, T.goal.offset, T.w_ctrl.offset, 3)


def test_rollout_kernel_has_no_spills_and_no_scratch(built, tmp_path):
    llvm = "/opt/rocm/lib/llvm/bin"
    for tool in ("llvm-objdump", "llvm-readelf"):  # (they come with the compiler that built the library)
        assert os.path.exists(llvm + "/" + tool), "%s is missing: the code object cannot be read" % tool
    shutil.copy(built, str(tmp_path / "l.so"))
    subprocess.run([llvm + "/llvm-objdump", "--offloading", "l.so"], cwd=str(tmp_path), check=True, capture_output=True)
    notes = "".join(subprocess.run([llvm + "/llvm-readelf", "--notes", f], cwd=str(tmp_path), check=True, capture_output=True, text=True).stdout
                    for f in os.listdir(str(tmp_path)) if "gfx950" in f)
    found = {}
    for m in re.finditer(r"\.name:\s+(\S+)\n(.*?)\.wavefront_size", notes, re.S):
        if "cartpole_rollout_kernel" in m.group(1):
            found[m.group(1)] = (int(re.search(r"\.vgpr_spill_count:\s+(\d+)", m.group(2)).group(1)),
                                 int(re.search(r"\.private_segment_fixed_size:\s+(\d+)", m.group(2)).group(1)))
    assert len(found) == 1 and list(found.values()) == [(0, 0)], found


# ---------------------------------------------------------------------------------------------- the host model
def test_host_step_is_the_reference_step_bit_for_bit(golden):
    """random states, actions beyond +-1, all seven parameters per row, some x_d = 0: the same torch operations in the same order"""
    from dust_amd.models import CartPoleModel

    g = golden("cartpole_step")
    f = torch.from_numpy
    assert (g["states"][:, 1] == 0).sum() >= 5 and (np.abs(g["actions"]) > 1).sum() >= 10
    m = CartPoleModel(dt=float(g["dt"]), uncertain_params=NAMES7)
    nxt = m.step(f(g["states"]), f(g["actions"]), m.params_to_dict(f(g["params"])))
    assert nxt.dtype == torch.float32 and np.array_equal(nxt.numpy(), g["next"])
    assert np.array_equal(CartPoleModel().step(f(g["states"]), f(g["actions"])).numpy(), g["next_nominal"])
    assert not np.array_equal(g["next"], g["next_nominal"])
    m = CartPoleModel()
    assert m.family == "cartpole" and m.dt == 0.05 and m.observation_space.dim == 4 and m.action_space.dim == 1
    assert float(m.action_space.low[0]) == -1.0 and float(m.action_space.high[0]) == 1.0
    assert tuple(m.params_dict) == NAMES7 and m.params_dict["mu_c"] == 0.5e-3 and m.params_dict["f_mag"] == 10.0


def cart_jacobian(state, action, par, dt, log):
    """d (x_d', th_d') / d (g, m_c, m_p, L, mu_c, mu_p, F) of one CartPoleModel.step in closed form, float64 [2, 7]; log: times the value"""
    g, mc, mp, L, muc, mup, F = (float(v) for v in par)
    a = float(np.clip(action, -1.0, 1.0))
    xd, th, w = float(state[1]), float(state[2]), float(state[3])
    s, c, sg, w2 = np.sin(th), np.cos(th), float(np.sign(xd)), w * w
    mass, pm = mc + mc, mp * L
    fac = (a * F + pm * s * w2 - muc * sg) / mass
    pf = mup * w / pm
    den0 = 4.0 / 3 - mp * c * c / mass
    den = L * den0
    tdd = (g * s - c * fac - pf) / den
    #            g    m_c                         m_p                 L                  mu_c        mu_p    F
    dfac = np.array([0.0, -fac / mc, L * s * w2 / mass, mp * s * w2 / mass, -sg / mass, 0.0, a / mass])
    dpf = np.array([0.0, 0.0, -pf / mp, -pf / L, 0.0, w / pm, 0.0])
    dden = np.array([0.0, L * mp * c * c / (mass * mc), -L * c * c / mass, den0, 0.0, 0.0, 0.0])
    dpm = np.array([0.0, 0.0, L, mp, 0.0, 0.0, 0.0])
    dnum = np.array([s, 0, 0, 0, 0, 0, 0.0]) - c * dfac - dpf
    dtdd = (dnum - tdd * dden) / den
    dxdd = dfac - (c / mass) * (dpm * tdd + pm * dtdd)
    dxdd[1] += pm * tdd * c / (mass * mc)
    J = np.stack([dxdd * dt, dtdd * dt])
    return J * np.asarray(par, np.float64)[None] if log else J


def test_closed_form_jacobian_matches_float64_autograd(golden):
    g = golden("cartpole_jac")
    n = g["states"].shape[0]
    assert (g["states"][:, 1] == 0).sum() >= 2 and (np.abs(g["actions"]) > 1).sum() >= 2
    for log in (False, True):
        ref = g["jac_log" if log else "jac_lin"]
        for i in range(n):
            J = cart_jacobian(g["states"][i], g["actions"][i, 0], g["params"][i], float(g["dt"]), log)
            e = np.abs(J - ref[i]).max() / np.abs(ref[i]).max()
            assert e < 1e-10, (log, i, e)
        # sign(x_d) = 0 kills the mu_c column
        assert np.all(ref[g["states"][:, 1] == 0][:, :, 4] == 0)


# ---------------------------------------------------------------------------------------------- the fixtures' caps and power
def _check_quantity(g, q, per_slice=False):
    tol = float(g["tol_" + q])
    assert TOL <= tol <= CAP, (q, tol)
    t64 = twin(g, q)
    if per_slice:
        d = max(elemerr(a, b) for a, b in zip(g[q], t64))
    else:
        d = elemerr(g[q], t64)
    slack = 0.0 if q + "_f64" in g else 1e-9  # (a twin stored as a binary16 difference: cartpole_cases.twin)
    assert 2.0 * d <= tol * (1 + 1e-12) + slack, (q, d, tol)


@pytest.mark.parametrize("name", ROLLOUT_NAMES)
def test_rollout_fixture_caps_and_power(golden, name):
    g, s = golden("cartpole_" + name), ROLLOUT_BY_TAG[name]
    for q in ROLLOUT_QUANT:
        _check_quantity(g, q)
    lead = lead_quantity(s)
    assert elemerr(g[lead + "_off"], g[lead]) >= 10 * float(g["tol_" + lead])
    assert g["costs"].shape == (s["S"], s["N"]) and g["states"].shape == (s["M"], s["S"], s["N"], s["H"] + 1, 4)
    assert 0.1 < float(g["clamped_fraction"]) < 0.3 and float(g["state"][1]) != 0.0
    if s["up"]:
        assert g["params"].shape == (s["M"], len(s["up"]))
    if name == "ragged":
        assert s["N"] * s["S"] == 333 and s["H"] % 2 == 1
    if name == "scalar":
        assert (s["N"] * s["S"]) % s["M"] != 0


@pytest.mark.parametrize("name", TICK_NAMES)
def test_tick_fixture_caps_and_power(golden, name):
    g = golden("cartpole_" + name)
    for q in TICK_QUANT:
        _check_quantity(g, q, per_slice=q in ("costs", "score", "phi", "theta_after"))
    assert elemerr(g["costs_off"], g["costs"][-1]) >= 10 * float(g["tol_costs"])
    assert int(np.argmax(g["p_weights"])) == int(np.argmax(g["p_weights_f64"]))
    assert np.array_equal(g["a_seq"], g["theta_after"][-1][int(np.argmax(g["p_weights"]))])


@pytest.mark.parametrize("name", NAMES)
def test_filter_fixture_caps_and_power(golden, name):
    g, s = golden("mpf_cartpole_" + name), BY_TAG[name]
    for q in QUANT:
        tol = float(g["tol_" + q])
        assert TOL <= tol <= CAP, (q, tol)
        assert g[q + "_f64"].dtype == np.float64
        assert 2.0 * elemerr(g[q], g[q + "_f64"]) <= tol * (1 + 1e-12), q
    assert float(g["tol_disp_2"]) <= CAP_DISP
    rms = lambda a: float(np.sqrt(np.mean(np.asarray(a, np.float64) ** 2)))
    assert abs(float(g["tol_disp_2"]) - float(g["tol_x_2"]) * rms(g["x_2"]) / rms(g["x_2"].astype(np.float64) - g["x0"])) < 1e-12
    assert rms(g["x_2"].astype(np.float64) - g["x0"]) >= 0.005 * rms(g["x_2"])  # two steps move the particles by >= 0.5 % of their rms
    off = g["phi0_off"]
    power = elemerr(off, g["phi0"][:off.shape[0]])
    assert power >= 10 * float(g["tol_phi0"]) and power >= 10 * float(g["tol_disp_2"]), power
    assert g["x0"].shape == (s["Mp"], len(s["up"])) and g["obs0"].shape == (4,) and g["action"].shape == (1,)
    assert np.array_equal(g["x0"], particles(s["up"], s["Mp"], s["log"], s["seed"], s["spread"], s["centre"]))
    if not s["log"]:
        assert s["bw"] >= 0.1  # (linear space below 0.1: the reference's own phi is outside the cap)
    if name == "xd_zero":
        assert g["obs0"][1] == 0.0
    if name == "sat":
        assert abs(float(g["action"][0])) > 1.0


def test_sweep_fixture_caps(golden):
    g = golden("mpf_cartpole_sweep")
    assert tuple(int(v) for v in g["sizes"]) == SWEEP_SIZES
    for Mp in SWEEP_SIZES:
        for q in ("phi0", "x_2", "grad_norms_2"):
            assert TOL <= float(g["tol_%s_%d" % (q, Mp)]) <= CAP, (Mp, q)
        assert float(g["tol_disp_2_%d" % Mp]) <= CAP_DISP, Mp
        assert g["phi0_%d" % Mp].shape == (Mp, 3) and g["disp_2_f64_%d" % Mp].shape == (Mp, 3)


# ---------------------------------------------------------------------------------------------- the filter's closed forms end to end
def mpf_phi(x, lik, prior_bw, bw):
    """MPF.phi (mpf.py:40-57) with the prior's means at the particles themselves"""
    diff = x[:, None, :] - x[None, :, :]
    q = (diff ** 2).sum(-1)
    w = np.exp(-0.5 * q / prior_bw ** 2)
    prior = -(w[:, :, None] * diff).sum(1) / w.sum(1)[:, None] / prior_bw ** 2
    k = np.exp(-q / bw ** 2 / 2.0)
    return -(k[:, :, None] * diff).sum(1) / bw ** 2 + k @ (lik + prior) / x.shape[0]


def _step64(state, action, par, dt):
    g, mc, mp, L, muc, mup, F = par
    a = np.clip(action, -1.0, 1.0)
    x, xd, th, w = state
    s, c = np.sin(th), np.cos(th)
    mass, pm = mc + mc, mp * L
    fac = (a * F + pm * s * w * w - muc * np.sign(xd)) / mass
    tdd = (g * s - c * fac - mup * w / pm) / (L * (4.0 / 3 - mp * c * c / mass))
    xdd = fac - pm * tdd * c / mass
    return np.array([x + xd * dt, xd + xdd * dt, th + w * dt, w + tdd * dt])


def _phi64(x0, up, log, fixed, dt, obs0, action, obs1, obs_std, bw):
    f = lambda a: np.asarray(a, np.float32).astype(np.float64)  # (the float64 run starts from the fp32 inputs, widened)
    x, past, act, obs = f(x0), f(obs0), float(f(action)[0]), f(obs1)
    val = np.exp(x) if log else x
    cols = [NAMES7.index(k) for k in up]
    lik = np.zeros_like(x)
    for i in range(x.shape[0]):
        par = np.array([fixed[k] for k in NAMES7], np.float64)
        par[cols] = val[i]
        e = obs - _step64(past, act, par, dt)
        J = cart_jacobian(past, act, par, dt, log)
        lik[i] = (J[0, cols] * e[1] + J[1, cols] * e[3]) / obs_std ** 2
    return mpf_phi(x, lik, float(bw), float(bw))


@pytest.mark.parametrize("name", NAMES)
def test_closed_form_phi_matches_float64_reference(golden, name):
    g, s = golden("mpf_cartpole_" + name), BY_TAG[name]
    assert tuple(str(g["uncertain"]).split(",")) == s["up"]
    fixed = dict(zip(NAMES7, (float(v) for v in g["fixed"])))
    got = _phi64(g["x0"], s["up"], bool(int(g["log_space"])), fixed, float(g["dt"]), g["obs0"], g["action"], g["obs1"], float(g["obs_std"]), float(g["bw"]))
    e = elemerr(got, g["phi0_f64"])
    print("%s: closed forms vs float64 autograd %.1e" % (name, e))
    assert e < 1e-6, e


def test_sweep_inputs_rebuild(golden):
    """x0 of the sweep is not stored: the seeded function gives the particles the generator ran on (checked through phi at two sizes)"""
    g = golden("mpf_cartpole_sweep")
    for Mp in (7, 257):
        s = sweep_scenario(Mp)
        x0 = particles(s["up"], Mp, s["log"], s["seed"], s["spread"], s["centre"])
        got = _phi64(x0, s["up"], s["log"], s["fixed"], s["dt"], g["obs0"], g["action"], g["obs1"], s["obs_std"], s["bw"])
        assert elemerr(got, g["phi0_f64_%d" % Mp]) < 1e-6  # (the twin is stored in fp32: 6e-8)


# ---------------------------------------------------------------------------------------------- the host layer
def test_recognise_accepts_and_refuses():
    from dust_amd.costs import PendulumQuadCos, QuadraticCost, recognise
    from dust_amd.models import CartPoleModel

    m = CartPoleModel()
    ok = QuadraticCost((0.1, 0, 0.2, 0), (1, 2, 3, 4), (5, 6, 7, 8), (0.5,))
    got = recognise(m, ok.inst_cost, ok.term_cost)
    assert got["w_quad_state"] == (1.0, 2.0, 3.0, 4.0) and got["w_quad_term"] == (5.0, 6.0, 7.0, 8.0) and got["w_quad_ctrl"] == (0.5,)
    assert got["goal"] == tuple(float(np.float32(v)) for v in (0.1, 0, 0.2, 0))
    assert recognise(m, *(lambda c: (c.inst_cost, c.term_cost))(QuadraticCost((0, 0, 0, 0), (1, 1, 1, 1))))["w_quad_ctrl"] == (0.0,)
    five = QuadraticCost((0, 0, 0, 0, 0), (1, 1, 1, 1, 1))
    with pytest.raises(ValueError):
        recognise(m, five.inst_cost, five.term_cost)
    two = QuadraticCost((0, 0, 0, 0), (1, 1, 1, 1), None, (0.1, 0.1))
    with pytest.raises(ValueError):
        recognise(m, two.inst_cost, two.term_cost)
    other = QuadraticCost((0, 0, 0, 0), (1, 1, 1, 1))
    with pytest.raises(NotImplementedError):
        recognise(m, ok.inst_cost, other.term_cost)  # (the two halves of one cost object)
    with pytest.raises(NotImplementedError):
        recognise(m, lambda s, a=None, **k: s.sum(-1), lambda s, **k: s.sum(-1))
    pq = PendulumQuadCos()
    with pytest.raises(NotImplementedError):
        recognise(m, pq.inst_cost, pq.term_cost)


def test_mirror_classes_refuse_unknown_names_and_more_than_four_columns():
    from dust_amd.backend import _cartpole_struct
    from dust_amd.controllers import MultiDISCO
    from dust_amd.costs import QuadraticCost
    from dust_amd.inference import MPF, GaussianLikelihood
    from dust_amd.models import CartPoleModel

    with pytest.raises(ValueError):
        CartPoleModel(uncertain_params=("length", "mass"))  # (the pendulum's name)
    with pytest.raises(ValueError):
        CartPoleModel(uncertain_params=("length", "length"))
    five = CartPoleModel(uncertain_params=NAMES7[:5])  # the host step takes any number; the device four
    with pytest.raises(ValueError):
        MPF(torch.ones(8, 5), GaussianLikelihood(torch.zeros(4), 0.05, five, log_space=False), bw=0.1, optimizer_class=torch.optim.SGD, lr=1e-4)
    cost = QuadraticCost((0, 0, 0, 0), (1, 1, 1, 1), None, (0.1,))
    ctrl = MultiDISCO(observation_space=five.observation_space, action_space=five.action_space, hz_len=4, action_samples=4, params_samples=2,
                      inst_cost_fn=cost.inst_cost, term_cost_fn=cost.term_cost, params_sampling=True, n_policies=2)
    pd = torch.distributions.Independent(torch.distributions.Normal(torch.ones(5), 0.1 * torch.ones(5)), 1)
    with pytest.raises(ValueError):
        ctrl.forward(torch.zeros(4), five, pd)
    vals = dict(g=9.8, f_mag=10.0, mass_cart=1.0, mass_pole=0.1, length=1.0, mu_c=5e-4, mu_p=2e-6)
    with pytest.raises(ValueError):
        _cartpole_struct(vals, ["length", "wheel_radius"])
    with pytest.raises(ValueError):
        _cartpole_struct(vals, list(NAMES7[:5]))
    st = _cartpole_struct(vals, ["mu_p", "g"])
    assert (st.mu_p.kind, st.mu_p.column, st.g.kind, st.g.column, st.length.kind) == (1, 0, 1, 1, 0) and st.f_mag.value == 10.0
