"""Which first pass a rollout launch takes (dust_amd.hip launch_rollout): the launch counts of the two profile slots after ONE
disco_forward / likelihood_sample call.  `states_kernel` counts the first pass (skid.hpp, cartpole.hpp, particle_general.hpp or a
whole-line stored-states kernel of rollout_states.hpp: rollouts + costs (+ states) into the staging buffer), `rollout_kernel` the
regular kernel (after a first pass: its injected-costs mode).  At most one first pass runs, and the regular kernel always does.

Only the path is pinned here: the counts, and that the costs came back finite.  The numbers stay with test_gpu_states_form.py,
test_gpu_ctrl_noise.py, test_gpu_cartpole.py and test_gpu_parity.py."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

S = 8
PARTICLE = dict(model="particle", with_obstacle=False, can_crash=False, alpha=1e-4, sigma_a=5.0, sigma_p=5.0)
PENDULUM = dict(model="pendulum", sigma_a=2.0, sigma_p=2.0)
NOISY = dict(PARTICLE, deterministic=False, noise_std=(0.6, 0.4), sigma_a=1.0, mass=2.0, dt=0.05, seed=5)
STATE = {"particle": [-5.2, -7.3, 4.0, 3.0], "pendulum": [3.0, -0.4], "skid_steer": [0.5, -0.3, 0.2, 0.0, 0.0], "cartpole": [0.1, 0.0, 0.05, 0.0]}
UNCERTAIN = {"particle": ("mass",), "pendulum": ("length", "mass"), "skid_steer": ("x_icr", "wheel_radius"), "cartpole": ("length", "mass_pole")}
PARAM_RANGE = {"particle": (0.6, 1.6), "pendulum": (0.6, 1.4), "skid_steer": (0.05, 0.2), "cartpole": (0.3, 0.9)}

# (id, context keywords, N, H, M, call, keywords of the call, environment, recorded control noise, (states_kernel, rollout_kernel))
CASES = [
    ("particle_states_N8_H8", PARTICLE, 8, 8, 2, "forward", dict(want_states=True), {}, False, (1, 1)),
    ("particle_states_N12_H10_ragged_group", PARTICLE, 12, 10, 2, "forward", dict(want_states=True), {}, False, (0, 1)),
    ("particle_states_N16_H11_even_rows", PARTICLE, 16, 11, 2, "forward", dict(want_states=True), {}, False, (0, 1)),
    ("particle_states_N8_H6_short", PARTICLE, 8, 6, 2, "forward", dict(want_states=True), {}, False, (0, 1)),
    ("particle_states_N8_H8_M1", PARTICLE, 8, 8, 1, "forward", dict(want_states=True), {}, False, (0, 1)),
    ("particle_states_N8_H8_form0", PARTICLE, 8, 8, 2, "forward", dict(want_states=True), {"DUST_STATES_FORM": "0"}, False, (0, 1)),
    ("particle_costs_only_N8_H8", PARTICLE, 8, 8, 2, "forward", dict(), {}, False, (0, 1)),
    ("particle_f16_N16_H16", PARTICLE, 16, 16, 2, "forward", dict(want_states=True, store_f16=True), {}, False, (1, 1)),
    ("particle_f16_N8_H16_ragged_group", PARTICLE, 8, 16, 2, "forward", dict(want_states=True, store_f16=True), {}, False, (0, 1)),
    ("particle_f16_N16_H14_short", PARTICLE, 16, 14, 2, "forward", dict(want_states=True, store_f16=True), {}, False, (0, 1)),
    ("pendulum_states_N16_H16", PENDULUM, 16, 16, 2, "forward", dict(want_states=True), {}, False, (1, 1)),
    ("pendulum_states_N16_H14_short", PENDULUM, 16, 14, 2, "forward", dict(want_states=True), {}, False, (0, 1)),
    ("pendulum_states_N16_H17_even_rows", PENDULUM, 16, 17, 2, "forward", dict(want_states=True), {}, False, (0, 1)),
    ("pendulum_states_N8_H16_ragged_group", PENDULUM, 8, 16, 2, "forward", dict(want_states=True), {}, False, (0, 1)),
    ("pendulum_f16_N32_H5", PENDULUM, 32, 5, 2, "forward", dict(want_states=True, store_f16=True), {}, False, (1, 1)),
    ("pendulum_f16_N16_H16_ragged_group", PENDULUM, 16, 16, 2, "forward", dict(want_states=True, store_f16=True), {}, False, (0, 1)),
    ("skid_steer_costs_only", dict(model="skid_steer", dt=0.1, sigma_a=0.3, sigma_p=0.3), 8, 8, 2, "sample", dict(), {}, False, (1, 1)),
    ("cartpole_costs_only", dict(model="cartpole", sigma_a=0.5, sigma_p=0.5), 8, 8, 2, "sample", dict(), {}, False, (1, 1)),
    ("particle_velocity_costs_only", dict(PARTICLE, control_type="velocity"), 8, 8, 2, "sample", dict(), {}, False, (1, 1)),
    ("ctrl_noise_drawn_inline", NOISY, 8, 8, 2, "sample", dict(), {}, False, (0, 1)),
    ("ctrl_noise_general_switch", NOISY, 8, 8, 2, "sample", dict(), {"DUST_NOISE_GENERAL": "1"}, False, (1, 1)),
    ("ctrl_noise_recorded_draws", NOISY, 8, 8, 2, "sample", dict(), {}, True, (1, 1)),
    ("ctrl_noise_states_wanted", NOISY, 8, 8, 2, "sample", dict(store_states=True), {}, False, (1, 1)),
]


@pytest.mark.parametrize("ctx,N,H,M,call,call_kw,env,recorded,want", [c[1:] for c in CASES], ids=[c[0] for c in CASES])
def test_first_pass_and_regular_kernel_launch_counts(ctx, N, H, M, call, call_kw, env, recorded, want, monkeypatch):
    from dust_amd import Context

    for k, v in env.items():  # (the development switches are read when the context is made)
        monkeypatch.setenv(k, v)
    model = ctx["model"]
    up = UNCERTAIN[model][: 1 if model == "particle" else 2] if M > 1 else None
    c = Context(N=N, S=S, M=M, H=H, uncertain_params=up, **ctx)
    rng = np.random.default_rng(100 * N + H)
    theta = (0.3 * rng.standard_normal((N, H, c.da))).astype(np.float32)
    noise = (0.5 * rng.standard_normal((S, N, H, c.da))).astype(np.float32)
    params = None if up is None else rng.uniform(*PARAM_RANGE[model], (M, len(up))).astype(np.float32)
    state = np.array(STATE[model][: c.ds], np.float32)
    c.set_theta(theta)
    c.set_a_mat(theta)
    if recorded:
        c.set_ctrl_noise(rng.standard_normal((1, H, M * S * N, 2)).astype(np.float32))
    c.profile(True)
    if call == "forward":
        costs = c.disco_forward(state, noise, params, **call_kw)[0]
    else:
        costs = c.likelihood_sample(state, noise, params, **call_kw)
    prof = c.profile_get()
    c.close()
    got = tuple(prof.get(k, (0.0, 0))[1] for k in ("states_kernel", "rollout_kernel"))
    assert got == want, prof
    assert costs.shape == (S, N) and np.isfinite(costs).all()
