"""The skid-steer dynamics filter without a GPU: the library exports its entry, the fixtures of tests/golden/make_golden_mpf_skid.py keep
their caps and their power, and a float64 numpy restatement of MPF.phi with the CLOSED-FORM one-step Jacobian (the forms mpf.hpp's
mpf_skid_score evaluates, written out again below) reproduces the reference's float64 autograd phi of every fixture."""
import ctypes as C

import numpy as np
import pytest

import __graft_entry__ as entry
from helpers import elemerr
from mpf_skid_cases import NAMES, NAMES3, SWEEP_SIZES, particles, sweep_scenario

CAP, CAP_DISP, TOL = 5e-5, 2e-3, 1e-5
QUANT = ("phi0", "x_2", "grad_norms_2", "x_n", "grad_norms", "x_n2", "grad_norms2", "probe_log_prob")


def test_library_exports_and_binds_the_skid_filter_entry():
    from dust_amd import _lib

    lib = C.CDLL(entry.build())
    assert hasattr(lib, "dust_mpf_set_skid_steer")
    assert "dust_mpf_set_skid_steer" in _lib.SYMBOLS
    assert _lib.SYMBOLS["dust_mpf_set_skid_steer"] == _lib.SYMBOLS["dust_set_skid_steer"]  # (handle, const dust_skid_config *)


@pytest.mark.parametrize("name", NAMES)
def test_fixture_caps_and_power(golden, name):
    g = golden("mpf_skid_" + name)
    for q in QUANT:
        tol = float(g["tol_" + q])
        assert TOL <= tol <= CAP, (q, tol)
        assert q + "_f64" in g and g[q + "_f64"].dtype == np.float64
        d = elemerr(g[q], g[q + "_f64"])  # the tolerance covers the reference's own fp32 / float64 distance twice
        assert 2.0 * d <= tol * (1 + 1e-12), (q, d, tol)
    assert float(g["tol_disp_2"]) <= CAP_DISP
    rms = lambda a: float(np.sqrt(np.mean(np.asarray(a, np.float64) ** 2)))
    assert abs(float(g["tol_disp_2"]) - float(g["tol_x_2"]) * rms(g["x_2"]) / rms(g["x_2"].astype(np.float64) - g["x0"])) < 1e-12
    off = g["phi0_off"]
    power = elemerr(off, g["phi0"][:off.shape[0]])
    assert power >= 10 * float(g["tol_phi0"]) and power >= 10 * float(g["tol_disp_2"]), power
    assert g["x0"].shape == (int(g["Mp"]), int(g["P"])) and g["obs0"].shape == (5,) and g["action"].shape == (2,)


def test_sweep_fixture_caps(golden):
    g = golden("mpf_skid_sweep")
    assert tuple(int(v) for v in g["sizes"]) == SWEEP_SIZES
    for Mp in SWEEP_SIZES:
        for q in ("phi0", "x_2", "grad_norms_2"):
            assert TOL <= float(g["tol_%s_%d" % (q, Mp)]) <= CAP, (Mp, q)
        assert float(g["tol_disp_2_%d" % Mp]) <= CAP_DISP, Mp
        assert g["phi0_%d" % Mp].shape == (Mp, 3) and g["disp_2_f64_%d" % Mp].shape == (Mp, 3)


# ---------------------------------------------------------------------------------------------- the closed forms, in float64 numpy
def skid_lik_score(x, up, log, fixed, lo, hi, dt, past, act, obs, obs_std):
    """J^T (obs - f(past, act; params)) / obs_std^2 per particle [Mp, P]: SkidSteerRobot.step and its parameter Jacobian in closed form"""
    val = np.exp(x) if log else x
    par = {k: (val[:, up.index(k)] if k in up else np.full(x.shape[0], fixed[k])) for k in NAMES3}
    xicr, wr, ad = par["x_icr"], par["wheel_radius"], par["axial_distance"]
    r, l = np.clip(act[0], lo[0], hi[0]), np.clip(act[1], lo[1], hi[1])
    c, s = np.cos(past[2]), np.sin(past[2])
    lin = (r + l) * np.pi * wr
    ang = 2.0 * np.pi * (r - l) * wr / ad
    fwd, lat = lin * dt, -ang * xicr * dt
    pred = np.stack([past[0] + fwd * c - lat * s, past[1] + fwd * s + lat * c, past[2] + ang * dt, lin, ang], 1)
    e = obs[None] - pred
    zero = np.zeros_like(wr)
    dang_w, dang_a = 2.0 * np.pi * (r - l) / ad, -ang / ad
    d = {  # (d lin, d ang, d lat) per parameter
        "x_icr": (zero, zero, -ang * dt),
        "wheel_radius": ((r + l) * np.pi + zero, dang_w, -xicr * dt * dang_w),
        "axial_distance": (zero, dang_a, -xicr * dt * dang_a),
    }
    out = np.zeros_like(x)
    for p, k in enumerate(up):
        dlin, dang, dlat = d[k]
        dfwd = dlin * dt
        col = (dfwd * c - dlat * s) * e[:, 0] + (dfwd * s + dlat * c) * e[:, 1] + dang * dt * e[:, 2] + dlin * e[:, 3] + dang * e[:, 4]
        out[:, p] = col * (par[k] if log else 1.0) / obs_std ** 2
    return out


def mpf_phi(x, lik, prior_bw, bw):
    """MPF.phi (mpf.py:40-57) with the prior's means at the particles themselves"""
    diff = x[:, None, :] - x[None, :, :]  # [i, j]
    q = (diff ** 2).sum(-1)
    w = np.exp(-0.5 * q / prior_bw ** 2)
    prior = -(w[:, :, None] * diff).sum(1) / w.sum(1)[:, None] / prior_bw ** 2
    k = np.exp(-q / bw ** 2 / 2.0)
    return -(k[:, :, None] * diff).sum(1) / bw ** 2 + k @ (lik + prior) / x.shape[0]


def _phi64(x0, up, log, fixed, lo, hi, dt, obs0, action, obs1, obs_std, bw):
    f = lambda a: np.asarray(a, np.float32).astype(np.float64)  # (the float64 run starts from the fp32 inputs, widened)
    x = f(x0)
    lik = skid_lik_score(x, up, log, fixed, f(lo), f(hi), float(dt), f(obs0), f(action), f(obs1), float(obs_std))
    return mpf_phi(x, lik, float(bw), float(bw))


@pytest.mark.parametrize("name", NAMES)
def test_closed_form_jacobian_matches_float64_autograd(golden, name):
    g = golden("mpf_skid_" + name)
    up = tuple(str(g["uncertain"]).split(","))
    fixed = dict(zip(NAMES3, (float(v) for v in g["fixed"])))
    got = _phi64(g["x0"], up, bool(int(g["log_space"])), fixed, g["min_a"], g["max_a"], g["dt"], g["obs0"], g["action"], g["obs1"], g["obs_std"], g["bw"])
    e = elemerr(got, g["phi0_f64"])
    print("%s: closed forms vs float64 autograd %.1e" % (name, e))
    assert e < 1e-6, e


def test_sweep_inputs_rebuild(golden):
    """x0 of the sweep is not stored: the seeded function gives the particles the generator ran on (checked through phi at two sizes)"""
    g = golden("mpf_skid_sweep")
    for Mp in (7, 257):
        s = sweep_scenario(Mp)
        x0 = particles(s["up"], Mp, s["log"], s["seed"], s["spread"])
        got = _phi64(x0, s["up"], s["log"], s["fixed"], s["lo"], s["hi"], s["dt"], g["obs0"], g["action"], g["obs1"], s["obs_std"], s["bw"])
        assert elemerr(got, g["phi0_f64_%d" % Mp]) < 1e-6  # (the twin is stored in fp32: 6e-8)
