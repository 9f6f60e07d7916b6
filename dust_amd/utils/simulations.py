"""Closed-loop drivers with the reference's entry points (dust/utils/simulations.py:13-260): `run_pendulum_simulation`
and `run_particle_episode`, same arguments, same per-tick call order, same result formats (the pendulum driver returns the
pandas frame demo/pendulum_example.py pickles to `data.pkl`; the particle driver returns the cumulated cost).

Everything on the hot path (svmpc.optimize / forward, controller.forward / step, mpf.optimize) runs on the MI355X through
the C ABI.  The PLANT is host code by nature (one state, one step per tick): the reference steps gym's `Pendulum-v0`,
which is not installable here, so the pendulum driver steps a `PendulumModel` carrying the episode's true (length, mass)
and gym's g = 10, max torque 2, max speed 8 (the same equations gym integrates); the particle driver steps a deep copy
of the controller's own `Particle`, as the reference does.  `render` is out of scope (plots)."""
from copy import deepcopy

import torch

from ..controllers.dual import DualSVMPC
from ..inference.likelihoods import ExponentiatedUtility
from ..inference.svmpc import SVMPC
from ..models import PendulumModel


def _nan(*shape):
    return torch.full(shape, float("nan"), dtype=torch.float)


def run_pendulum_simulation(init_state, init_policies, model_kwargs, dyn_dist, experiment_params, controller, use_exact_model=True,
                            use_svmpc=True, svmpc_kwargs=None, lik_kwargs=None, mpf=None, mpf_bw=None, mpf_steps=20, episodes=3,
                            steps=200, render=False, warm_up=1, verbose=False, steps_per_message=20):
    import pandas as pd

    if render:
        raise NotImplementedError("render: plotting is out of scope for the MI355X build")
    frames = []
    for ep in range(episodes):
        truth = experiment_params[ep]
        print("--- Starting iteration {} ---".format(ep + 1))
        print("parameters are: " + " and ".join("{} {:.2f}".format(k, float(v)) for k, v in truth.items()))
        if use_exact_model:
            model = PendulumModel(**truth, **model_kwargs)
        else:
            model = PendulumModel(length=dyn_dist.mean[0], mass=dyn_dist.mean[1], **model_kwargs)
        plant = PendulumModel(g=10.0, length=float(truth["length"]), mass=float(truth["mass"]))  # gym Pendulum-v0 stand-in
        state = torch.as_tensor(init_state, dtype=torch.float).reshape(1, -1)
        # the controller of this episode: same starting plan as SVMPC's particles, separate storage (simulations.py:60-63)
        sim_ctrl = deepcopy(controller)
        sim_ctrl.a_mat = init_policies.detach().clone()
        sim_ctrl.return_rollouts = False  # nothing below reads the sampled states / actions (no rendering)
        sim_svmpc = None
        if use_svmpc:
            if svmpc_kwargs is None or lik_kwargs is None:
                raise AssertionError("Need a Stein Optimizer and likelihood for dual svmpc simulation.")
            sim_svmpc = SVMPC(likelihood=ExponentiatedUtility(**lik_kwargs, controller=sim_ctrl, model=model), **svmpc_kwargs)
        sim_mpf, dyn_particles, dyn_bws = None, None, None
        ep_dyn_dist = dyn_dist
        if mpf is not None:
            sim_mpf = deepcopy(mpf)
            ep_dyn_dist = sim_mpf.prior
            dyn_particles = _nan(steps, *sim_mpf.x.size())
            dyn_bws = torch.zeros(steps)
        # the two inferences of the dual loop as one object (controllers/dual.py): forward() = optimize (+ forward once warmed up,
        # simulations.py:108-123), step() = the filter update (simulations.py:132-138)
        dual = DualSVMPC(sim_svmpc, sim_mpf, dyn_dist=ep_dyn_dist, mpf_bw=mpf_bw, mpf_steps=mpf_steps, warm_up=warm_up) if use_svmpc else None
        states, actions, costs = _nan(steps, sim_ctrl.dim_s), _nan(steps, sim_ctrl.dim_a), _nan(steps, 1)
        pol_particles = _nan(steps, sim_ctrl.n_pol, sim_ctrl.hz_len, sim_ctrl.dim_a)
        weights = _nan(steps, sim_ctrl.n_pol)
        action, cost = torch.zeros(sim_ctrl.dim_a), torch.zeros(1)
        for step in range(steps):
            if use_svmpc:
                a_seq, p_weights = dual.forward(state)
                action = a_seq[0]
                if p_weights is not None:
                    pol_particles[step] = dual.theta.detach().clone()
                    weights[step] = p_weights
            else:
                sim_ctrl.forward(state, model, ep_dyn_dist)
                action = sim_ctrl.step(strategy="average").flatten()
            actions[step] = action
            state = plant.step(state, torch.as_tensor(action, dtype=torch.float).clamp(-2.0, 2.0).reshape(1, -1)).reshape(1, -1)
            if sim_mpf is not None:
                if dual is not None:
                    _, bw = dual.step(action, state)
                else:
                    _, bw = sim_mpf.optimize(action.squeeze(), state, bw=mpf_bw, n_steps=mpf_steps)
                dyn_particles[step] = sim_mpf.x
                dyn_bws[step] = bw
            cost = sim_ctrl.inst_cost_fn(state.view(1, -1))
            if verbose and not step % steps_per_message:
                print("Step {0}: action taken {1:.2f}, cost {2:.2f}".format(step, float(action), float(cost)))
                print("Current state: theta={0[0]}, theta_dot={0[1]}".format(state.squeeze()))
            states[step] = state
            costs[step] = cost
        if verbose:
            print("Last step {0}: action taken {1:.2f}, cost {2:.2f}".format(steps - 1, float(action), float(cost)))
        # column set of the reference's frame (simulations.py:171-190); it hard-codes 200 rows, here: `steps`
        df = pd.DataFrame(index=list(range(steps)), data={
            "Cost": costs[:, 0].numpy(), "Position": states[:, 0].numpy(), "Speed": states[:, 1].numpy(), "Actions": actions[:, 0].numpy(),
            "Timestep": torch.arange(steps).numpy(), "Iteration": ep,
            "DynParticles": dyn_particles.tolist() if dyn_particles is not None else None,
            "DynBandwidths": None if dyn_bws is None else dyn_bws.numpy(),
            "PolParticles": pol_particles[..., 0, 0].tolist(), "Weights": weights.tolist(),
            "ExpParams": steps * [list(truth.values())],
        })
        df["AvgCumCost"] = (df["Cost"].cumsum(0) / (df["Timestep"] + 1)).round(2)
        frames.append(df)
    return pd.concat(frames, axis=0) if frames else pd.DataFrame()


def run_particle_episode(init_state, model, dyn_dist, controller, use_svmpc=True, warm_up=30, svmpc=None, load=0, steps=400,
                         render=False, save_path=None, mpf=None, mpf_bw=None, mpf_steps=20, verbose=False):
    """Point-mass navigation episode: the simulated system starts as a copy of `model`; after a quarter of the episode its
    mass grows by `load` (simulations.py:208-209).  Ends on a crash (cost inf), within 1.0 of the target, or after `steps`.
    `mpf` (optional, as particle_example.py:196-203 does inline): the dynamics filter updated after every plant step;
    pass `dyn_dist = mpf.prior` with it."""
    if render:
        raise NotImplementedError("render: plotting is out of scope for the MI355X build")
    system = deepcopy(model)
    controller.return_rollouts = False  # the sampled states only feed the (unsupported) renderer
    state = torch.as_tensor(init_state, dtype=torch.float).clone()
    cum_cost = 0
    for step in range(steps):
        if step == steps // 4:
            system.params_dict["mass"] = system.params_dict["mass"] + load
        if use_svmpc:
            svmpc.optimize(state, dyn_dist)
            if step < warm_up:
                action = torch.zeros(controller.dim_a)
            else:
                a_seq, _ = svmpc.forward(state, dyn_dist)
                action = a_seq[0]
        else:
            controller.forward(state, model, params_dist=dyn_dist)
            action = controller.step(strategy="argmax")
        new_state = system.step(state, action.squeeze())
        if mpf is not None:
            mpf.optimize(action.squeeze(), new_state, bw=mpf_bw, n_steps=mpf_steps)
        state = new_state
        cost = controller.inst_cost_fn(state.view(1, -1))
        cum_cost = cum_cost + cost
        if verbose and step % 10 == 0:
            print("step %3d  pos (%.2f, %.2f)  vel (%.2f, %.2f)  cost %.1f" % (step, *[float(v) for v in state], float(cost)))
        if system.with_obstacle and bool(system.obst_map.get_collisions(state[:2])):
            print("Crashed at step {}".format(step))
            return float("inf")
        if float((system.target - state).norm()) <= 1.0:
            break
    return cum_cost


_PIECE = 4096  # the periods one device episode call takes: a longer episode is a chain of pieces


def posterior_history_columns(theta_pieces, x_pieces, final_x, warm_up, n_run=None):
    """The reference frame's `PolParticles` / `DynParticles` columns (simulations.py:122, 134-137) from the rows the device episodes
    record - a pure host function over arrays.  theta_pieces: the pieces' `theta` histories [T_i, B, N, H, da] in episode order;
    x_pieces: their filter histories [T_i, B, Mp, P] - row t holds the filter period t's tick drew from, that is BEFORE the pair of
    period t is folded in; final_x [B, Mp, P]: the filters with the episode's last pair folded in (`dual.dyn_particles`); warm_up: the
    episode's warm-up periods; n_run [B]: the periods every environment ran (None: all of them).
    -> (DynParticles [B, steps, Mp, P], PolParticles [B, steps, N]):
       PolParticles[:, t] = theta[..., 0, 0] after period t, NaN while the episode warms up (the reference stores a row only behind a
       forward());
       DynParticles[:, t] = the filter after it folded in the pair of period t: row t + 1 of the recording - across a piece's end row 0
       of the next piece, whose update runs from the noted pair - and, for an environment's last period, final_x.
    Rows past n_run[b] are NaN."""
    import numpy as np

    theta = np.concatenate([np.asarray(v, np.float32) for v in theta_pieces])  # [steps, B, N, H, da]
    x = np.concatenate([np.asarray(v, np.float32) for v in x_pieces])          # [steps, B, Mp, P]
    final_x = np.asarray(final_x, np.float32)
    steps, B = theta.shape[:2]
    if x.shape[:2] != (steps, B) or final_x.shape != x.shape[1:]:
        raise ValueError("histories of %s and %s rows, final particles %s" % (theta.shape[:2], x.shape[:2], final_x.shape))
    n_run = np.full(B, steps, np.int64) if n_run is None else np.asarray(n_run, np.int64).reshape(B)
    pol = theta[..., 0, 0].transpose(1, 0, 2).copy()  # [B, steps, N]
    pol[:, :min(int(warm_up), steps)] = np.nan
    dyn = np.full((B, steps) + x.shape[2:], np.nan, np.float32)
    dyn[:, :steps - 1] = x[1:].transpose(1, 0, 2, 3)
    for b in range(B):
        n = int(min(max(n_run[b], 0), steps))
        dyn[b, n:], pol[b, n:] = np.nan, np.nan
        if n > 0:
            dyn[b, n - 1] = final_x[b]
    return dyn, pol


def run_pendulum_simulations(init_state, init_policies, model_kwargs, experiment_params, controller, svmpc_kwargs, lik_kwargs, mpf, mpf_bw=None,
                             mpf_steps=20, episodes=3, steps=200, warm_up=1, seed=0, init_particles=None, frame=False, *, use_svmpc=True,
                             dyn_dist=None, use_exact_model=False, mpf_hyper=None, history=False):
    """The batched twin of `run_pendulum_simulation(use_svmpc=True, mpf=...)`: the `episodes` become the B environments of one
    `BatchSVMPC` plus `BatchDualSVMPC`, environment i's plant runs under `experiment_params[i]`, and the whole loop - warm-up periods
    that only optimize and apply a zero action while the filters keep updating, the cost of every new state - runs on the device, one
    `BatchDualSVMPC.simulate` call per piece of at most 4096 periods.  `svmpc_kwargs` are SVMPC's keywords (init_particles, prior, ...;
    `seeds` too), `lik_kwargs` ExponentiatedUtility's, `mpf` the filter prototype every environment copies (`init_particles`
    [B, Mp, P]: its own start), `seed` the base of the filters' prior keys.  `mpf_hyper` (keyword only): B filter rows - dicts or a
    structured array with any of lr, obs_std, bw, bw_scale (`BatchDualSVMPC.set_filter_hyper`) - the trials of a sweep over the filter's
    settings, one per environment; `mpf_bw` must then be None (the rows carry the bandwidths).

    The plants.  They step the CONTROLLER'S model - `PendulumModel(**model_kwargs)`, the model of all B environments - under the true
    rows: the columns of its `uncertain_params`, from `experiment_params[i]` (a name it lacks keeps the model's value), without noise and
    with the action clamped as the rollouts clamp it.  The lone driver's plant is a stand-in for gym's Pendulum-v0 with g = 10;
    `model_kwargs=dict(g=10.0, ...)` gives this driver the same equations.  The nominal values of the uncertain parameters are never
    read: every dynamics sample is drawn from the environment's filter.

    -> a dict of arrays under the reference frame's column names, [B, steps] unless stated: `Cost`, `Position`, `Speed`, `Actions`,
    `Timestep`, `Iteration`, `DynBandwidths`, `Weights` [B, steps, N] (NaN while warming up), `ExpParams` [B, steps, P], `AvgCumCost`,
    and - the episode is not interrupted to read them - `DynParticles` [B, Mp, P] and `PolParticles` [B, N]: the FINAL filter particles
    (the last pair folded in) and the final particles' first actions, not one row per period.  history=True (keyword only): one row
    per period, as the reference's frame has them - `DynParticles` [B, steps, Mp, P], the filter after it folded in the pair of period
    t, and `PolParticles` [B, steps, N], the particles' first actions after period t (NaN while warming up) - recorded by the episodes'
    own kernels (`BatchDualSVMPC.set_history`): still no interruption, no launch more.  frame=True: the reference's pandas
    frame of the per-period columns, when pandas imports (it is optional here); otherwise the dict.

    use_svmpc=False (keyword only): the `use_svmpc=False` branch of the lone driver (simulations.py:124-126) - the MPPI-baseline and DISCO
    cases of demo/pendulum_example.py - as one `BatchDISCO.simulate` per piece: `controller` is a `BatchDISCO` of `episodes` environments
    (params_sampling=None: the baseline; a MerweScaledUTF: DISCO, whose sigma points are `dyn_dist`'s, fixed over the episode), every
    period forward + step("average"); `svmpc_kwargs`, `lik_kwargs` and `mpf` are not read and may be None, and there is no warm-up.
    use_exact_model=True (the demo's baseline): every environment's rollouts run under ITS true row - the controller then has
    params_sampling=True with params_samples=1, and the row it "samples" is the truth.  The
    dict then has no `DynParticles` / `DynBandwidths` / `Weights`, and `PolParticles` are the final plans' first actions."""
    import numpy as np

    if not use_svmpc:
        return _run_pendulum_baselines(init_state, init_policies, model_kwargs, experiment_params, controller, dyn_dist, int(episodes), int(steps), frame,
                                       bool(use_exact_model))
    from ..controllers.dual import BatchDualSVMPC
    from ..inference.svmpc import BatchSVMPC

    B, steps = int(episodes), int(steps)
    if len(experiment_params) < B:
        raise ValueError("experiment_params has %d entries for %d episodes" % (len(experiment_params), B))
    model = PendulumModel(**model_kwargs)
    names = tuple(model.uncertain_params or ())
    if not names:
        raise ValueError("the dual loop estimates the model's uncertain_params: model_kwargs names none")
    sim_ctrl = deepcopy(controller)
    sim_ctrl.a_mat = init_policies.detach().clone()
    sim_ctrl.return_rollouts = False
    sv = BatchSVMPC(B, likelihood=ExponentiatedUtility(**lik_kwargs, controller=sim_ctrl, model=model), **svmpc_kwargs)
    dual = BatchDualSVMPC(sv, mpf, mpf_bw=mpf_bw, mpf_steps=mpf_steps, seed=seed, init_particles=init_particles, warm_up=warm_up)
    if mpf_hyper is not None:
        dual.set_filter_hyper(mpf_hyper)
    if history:
        dual.set_history(theta=True, filter=True)
    true = torch.tensor([[float(experiment_params[i].get(k, model.params_dict[k])) for k in names] for i in range(B)], dtype=torch.float)
    rows = true.log() if bool(sim_ctrl._params_log_space) else true
    state = torch.as_tensor(init_state, dtype=torch.float).reshape(1, -1).repeat(B, 1)
    out, res, hist = [], None, []
    for lo in range(0, steps, _PIECE):
        res = dual.simulate(state, min(_PIECE, steps - lo), plant_params=rows, resume=res)
        out.append(res)
        if history:
            hist.append(dual.history)
        state = res.states[-1]
    cat = lambda k: torch.cat([getattr(r, k) for r in out]).transpose(0, 1).numpy()  # [B, steps, ...]
    xs, cost = cat("states"), cat("costs")
    t = np.broadcast_to(np.arange(steps), (B, steps))
    data = {"Cost": cost, "Position": xs[..., 0], "Speed": xs[..., 1], "Actions": cat("actions")[..., 0], "Timestep": t.copy(),
            "Iteration": np.broadcast_to(np.arange(B)[:, None], (B, steps)).copy(), "DynParticles": dual.dyn_particles.numpy(),
            "DynBandwidths": cat("bw"), "PolParticles": dual.theta[:, :, 0, 0].numpy(), "Weights": cat("p_weights"),
            "ExpParams": np.broadcast_to(true.numpy()[:, None], (B, steps, len(names))).copy(),
            "AvgCumCost": np.round(np.cumsum(cost.astype(np.float64), 1) / (t + 1), 2)}
    if history:
        data["DynParticles"], data["PolParticles"] = posterior_history_columns(
            [h["theta"].numpy() for h in hist], [h["dyn_particles"].numpy() for h in hist], data["DynParticles"], warm_up)
    if frame:
        try:
            import pandas as pd
        except ImportError:
            return data
        per = ("Cost", "Position", "Speed", "Actions", "Timestep", "Iteration", "DynBandwidths", "AvgCumCost")
        cols = {k: data[k].reshape(-1) for k in per}
        cols["Weights"], cols["ExpParams"] = data["Weights"].reshape(B * steps, -1).tolist(), data["ExpParams"].reshape(B * steps, -1).tolist()
        return pd.DataFrame(index=list(t.reshape(-1)), data=cols)
    return data


def _run_pendulum_baselines(init_state, init_policies, model_kwargs, experiment_params, controller, dyn_dist, B, steps, frame, exact):
    """run_pendulum_simulations(use_svmpc=False): the episodes as the environments of a `BatchDISCO`"""
    import numpy as np

    from ..controllers.disco import BatchDISCO

    if not isinstance(controller, BatchDISCO) or controller.n_envs != B:
        raise ValueError("use_svmpc=False runs the episodes as the environments of one BatchDISCO: pass one of %d environments" % B)
    if len(experiment_params) < B:
        raise ValueError("experiment_params has %d entries for %d episodes" % (len(experiment_params), B))
    model = PendulumModel(**model_kwargs)
    sampled = bool(controller._sampling)
    names = tuple(model.uncertain_params or ()) if sampled else ()
    sim_ctrl = deepcopy(controller)
    init = torch.as_tensor(init_policies, dtype=torch.float).detach().clone()
    sim_ctrl.a_mat = init if init.ndim == 4 else init[None].repeat(B, 1, 1, 1)
    true = torch.tensor([[float(experiment_params[i].get(k, model.params_dict[k])) for k in names] for i in range(B)], dtype=torch.float).reshape(B, len(names))
    rows = None if not names else (true.log() if bool(sim_ctrl._params_log_space) else true)
    known = None
    if exact:
        if rows is None or sim_ctrl._tf is not None or sim_ctrl.n_params != 1:
            raise ValueError("use_exact_model=True hands every environment its true row: a BatchDISCO with params_sampling=True, "
                             "params_samples=1 over a model with uncertain_params")
        known = rows[:, None, :]  # [B, 1, P]: serves every period
    state = torch.as_tensor(init_state, dtype=torch.float).reshape(1, -1).repeat(B, 1)
    out, res = [], None
    for lo in range(0, steps, 4096):
        res = sim_ctrl.simulate(state, model, dyn_dist, min(4096, steps - lo), "average", plant_params=rows, resume=res, params=known)
        out.append(res)
        state = res.states[-1]
    cat = lambda k: torch.cat([getattr(r, k) for r in out]).transpose(0, 1).numpy()  # [B, steps, ...]
    xs, cost = cat("states"), cat("costs")
    t = np.broadcast_to(np.arange(steps), (B, steps))
    data = {"Cost": cost, "Position": xs[..., 0], "Speed": xs[..., 1], "Actions": cat("actions")[..., 0], "Timestep": t.copy(),
            "Iteration": np.broadcast_to(np.arange(B)[:, None], (B, steps)).copy(), "PolParticles": sim_ctrl.a_mat[:, :, 0, 0].numpy(),
            "ExpParams": np.broadcast_to(true.numpy()[:, None], (B, steps, len(names))).copy(),
            "AvgCumCost": np.round(np.cumsum(cost.astype(np.float64), 1) / (t + 1), 2)}
    if frame:
        try:
            import pandas as pd
        except ImportError:
            return data
        per = ("Cost", "Position", "Speed", "Actions", "Timestep", "Iteration", "AvgCumCost")
        cols = {k: data[k].reshape(-1) for k in per}
        cols["ExpParams"] = data["ExpParams"].reshape(B * steps, -1).tolist()
        return pd.DataFrame(index=list(t.reshape(-1)), data=cols)
    return data


def _particle_plants(model, sampling, log_space, plant_params, load, B):
    """(rows, loaded rows) [B, P] of run_particle_episodes' plants: the true rows (None: nominal) and, with `load` != 0, the rows from
    steps // 4 on - the mass grown by `load`"""
    rows = None if plant_params is None else torch.as_tensor(plant_params, dtype=torch.float).reshape(B, -1).clone()
    loaded = rows
    if load != 0:
        names = tuple(model.uncertain_params or ()) if sampling else ()
        if "mass" not in names:
            raise ValueError("load != 0 changes the plants' mass: 'mass' must be one of the model's uncertain parameters")
        if rows is None:
            nominal = torch.tensor([float(model.params_dict[k]) for k in names])
            rows = (nominal.log() if log_space else nominal).repeat(B, 1)
        j = names.index("mass")
        loaded = rows.clone()
        loaded[:, j] = (rows[:, j].exp() + load).log() if log_space else rows[:, j] + load
    return rows, loaded


def _run_particle_amppi(init_states, model, ctrl, load, steps, plant_params, mpf, mpf_bw, mpf_steps, details):
    """run_particle_episodes with a `BatchAMPPI`: run_particle_episode's use_svmpc=False branch under AMPPI - update_actions, the plant's
    step, roll(1) per period, no warm-up - on `BatchAMPPI.simulate`, or with `mpf` the dual loop on `BatchDualAMPPI.simulate`"""
    import numpy as np

    B = ctrl.n_envs
    state = torch.as_tensor(init_states, dtype=torch.float).reshape(B, -1).clone()
    sampling = ctrl._tf is not None or bool(ctrl._sample_shape)
    rows, loaded = _particle_plants(model, sampling, False, plant_params, load, B)
    dual = None
    if mpf is not None:
        from ..controllers.dual import BatchDualAMPPI

        dual = BatchDualAMPPI(ctrl, model, mpf, mpf_bw=mpf_bw, mpf_steps=mpf_steps)
    cuts = sorted({0, steps} | ({min(steps // 4, steps)} if load != 0 else set()) | set(range(0, steps, 4096)))
    crash = bool(model.with_obstacle)
    res, ran = None, torch.zeros(B, dtype=torch.int32)
    for lo, hi in zip(cuts[:-1], cuts[1:]):
        plant = loaded if (load != 0 and lo >= steps // 4) else rows
        kw = dict(goal=model.target, goal_radius=1.0, stop_on_crash=crash, plant_params=plant, resume=res)
        res = dual.simulate(state, hi - lo, **kw) if dual is not None else ctrl.simulate(model, state, hi - lo, **kw)
        n = res.n_run.numpy()
        for b in np.nonzero(n > 0)[0]:
            state[b] = res.states[n[b] - 1, b]
        ran += res.n_run.clamp(min=0)
    loss = res.loss if res is not None else torch.zeros(B)
    return (loss, res.status if res is not None else torch.zeros(B, dtype=torch.int32), ran) if details else loss


def _run_particle_baselines(init_states, model, dyn_dist, ctrl, load, steps, plant_params):
    """run_particle_episodes with a `BatchDISCO`: run_particle_episode's use_svmpc=False branch, step("argmax"), no warm-up"""
    import numpy as np

    B = ctrl.n_envs
    state = torch.as_tensor(init_states, dtype=torch.float).reshape(B, -1).clone()
    rows, loaded = _particle_plants(model, ctrl._sampling, bool(ctrl._params_log_space), plant_params, load, B)
    cuts = sorted({0, steps} | ({min(steps // 4, steps)} if load != 0 else set()) | set(range(0, steps, 4096)))
    res = None
    for lo, hi in zip(cuts[:-1], cuts[1:]):
        plant = loaded if (load != 0 and lo >= steps // 4) else rows
        res = ctrl.simulate(state, model, dyn_dist, hi - lo, "argmax", goal=model.target, goal_radius=1.0, stop_on_crash=bool(model.with_obstacle),
                            plant_params=plant, resume=res)
        n = res.n_run.numpy()
        for b in np.nonzero(n > 0)[0]:
            state[b] = res.states[n[b] - 1, b]
    return res.loss if res is not None else torch.zeros(B)


def run_particle_episodes(init_states, model, dyn_dist, batch_svmpc, warm_up=30, load=0, steps=400, plant_params=None, mpf=None, mpf_bw=None,
                          mpf_steps=20, mpf_hyper=None, *, details=False):
    """The batched twin of `run_particle_episode`: environment b of `batch_svmpc` (a `BatchSVMPC` over `model`) runs that episode from
    init_states[b] on the device (`BatchSVMPC.simulate`: warm-up, accumulated cost, crash - when the model has obstacles - and the goal
    `model.target` within 1.0), in pieces of at most 4096 periods.  The plants are deterministic and step under `plant_params` [B, P]
    (the columns and the space of the controller's dynamics samples; None: the nominal model); with `load` != 0 the episode is split at
    steps // 4 and the true mass grows by `load` from there on, which needs `mass` among the model's uncertain parameters.
    `mpf` (a filter prototype, as run_particle_episode's): the episode is the DuSt-MPC loop - every environment a copy of the filter,
    updated after every plant step, the warm-up periods included, and stopped with its environment - on `BatchDualSVMPC.simulate`;
    the dynamics samples then come from the filters (`dyn_dist` is not read).  The `load` split stays two calls.  `mpf_hyper`: B filter
    rows (`BatchDualSVMPC.set_filter_hyper`), one per environment; needs `mpf`, and `mpf_bw` must then be None.
    `batch_svmpc` may be a `BatchDISCO` instead: the episode is run_particle_episode's `use_svmpc=False` branch - every period forward +
    step("argmax"), no warm-up (`warm_up` is not read), no filter (`mpf` must be None) - on `BatchDISCO.simulate`.
    Or a `BatchAMPPI`: that branch under AMPPI - update_actions, the plant's step, roll(1); `warm_up` and `dyn_dist` are not read (the
    controller draws from `model.params_dist`) - on `BatchAMPPI.simulate`, and with `mpf` the dual loop on `BatchDualAMPPI.simulate`.
    details=True (keyword only, a `BatchAMPPI`): -> (losses [B], statuses [B]: 0 running, 1 goal, 2 crash; periods run [B]).
    -> losses [B]: the cumulated cost of every environment, inf after a crash."""
    import numpy as np

    from ..controllers.amppi import BatchAMPPI
    from ..controllers.disco import BatchDISCO

    if isinstance(batch_svmpc, BatchDISCO):
        if mpf is not None:
            raise ValueError("a BatchDISCO episode has no dynamics filter: mpf must be None")
        return _run_particle_baselines(init_states, model, dyn_dist, batch_svmpc, load, int(steps), plant_params)
    if isinstance(batch_svmpc, BatchAMPPI):
        if mpf_hyper is not None:
            raise ValueError("per-environment filter rows are the DuSt-MPC loop's: mpf_hyper must be None under a BatchAMPPI")
        return _run_particle_amppi(init_states, model, batch_svmpc, load, int(steps), plant_params, mpf, mpf_bw, mpf_steps, bool(details))
    if details:
        raise ValueError("details=True reports the statuses and periods of a BatchAMPPI episode")
    if mpf_hyper is not None and mpf is None:
        raise ValueError("mpf_hyper are the rows of the filters: pass the filter prototype as mpf")
    ctrl = batch_svmpc.likelihood.controller
    B = batch_svmpc.n_envs
    state = torch.as_tensor(init_states, dtype=torch.float).reshape(B, -1).clone()
    steps = int(steps)
    rows, loaded = _particle_plants(model, ctrl._sampling, bool(ctrl._params_log_space), plant_params, load, B)
    cuts = sorted({0, steps} | ({min(steps // 4, steps)} if load != 0 else set()) | set(range(0, steps, 4096)))
    crash = bool(model.with_obstacle)
    res = None
    dual = None
    if mpf is not None:
        from ..controllers.dual import BatchDualSVMPC

        dual = BatchDualSVMPC(batch_svmpc, mpf, mpf_bw=mpf_bw, mpf_steps=mpf_steps, warm_up=warm_up)
        if mpf_hyper is not None:
            dual.set_filter_hyper(mpf_hyper)
    for lo, hi in zip(cuts[:-1], cuts[1:]):
        plant = loaded if (load != 0 and lo >= steps // 4) else rows
        if dual is not None:
            res = dual.simulate(state, hi - lo, goal=model.target, goal_radius=1.0, stop_on_crash=crash, plant_params=plant, resume=res)
        else:
            res = batch_svmpc.simulate(state, dyn_dist, hi - lo, warm_up=warm_up, goal=model.target, goal_radius=1.0, stop_on_crash=crash,
                                       plant_params=plant, resume=res)
        n = res.n_run.numpy()
        for b in np.nonzero(n > 0)[0]:
            state[b] = res.states[n[b] - 1, b]
    return res.loss if res is not None else torch.zeros(B)
