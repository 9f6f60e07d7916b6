"""`MultiDISCO` with the reference's constructor, attributes and `forward` / `step` signatures
(dust/controllers/disco.py:8-417, dust/controllers/base.py:7-66), executing on the MI355X through the C ABI.

The controller OWNS the device context (one dust_ctx): rollouts, costs, weights and - when an SVMPC is attached - the Stein
particles and prior live there.  `copy.deepcopy(controller)` clones the context (dust_clone), as the simulation loops
require (simulations.py:62, particle_example.py:166-175)."""
import collections
import copy

import numpy as np
import torch

from .. import _lib as L
from ..backend import Context
from ..costs import cost_grid, cost_grid_key, recognise
from ..utils.utf import MerweScaledUTF

Empty = torch.Size([])


class MultiDISCO:
    def __init__(self, observation_space, action_space, hz_len, n_policies, action_samples, temperature=1.0, ctrl_penalty=1.0,
                 a_cov=None, inst_cost_fn=None, term_cost_fn=None, params_sampling=True, params_samples=4, params_log_space=False,
                 init_actions=None, **kwargs):
        self.hz_len = hz_len
        self.dim_s, self.dim_a = observation_space.dim, action_space.dim
        self.min_a, self.max_a = action_space.low, action_space.high
        if inst_cost_fn is None and term_cost_fn is None:
            raise ValueError("Specify at least one cost function")
        self.inst_cost_fn, self.term_cost_fn = inst_cost_fn, term_cost_fn
        self.n_pol, self.n_actions = n_policies, action_samples
        self.temp = temperature
        self.a_reg = temperature * (1 - ctrl_penalty)
        self._ctrl_penalty = ctrl_penalty
        if a_cov is None:
            a_cov = torch.eye(self.dim_a)
        a_cov = torch.as_tensor(a_cov, dtype=torch.float)
        if not torch.equal(a_cov, torch.diag(torch.diag(a_cov))) and self.dim_a != 2:
            raise NotImplementedError("a full a_cov has a HIP kernel for dim_a = 2 (no CPU fallback)")
        self.a_dist = torch.distributions.multivariate_normal.MultivariateNormal(torch.zeros(self.dim_a), a_cov)
        self.a_pre = torch.inverse(a_cov)
        self._a_seq = torch.zeros((hz_len, self.dim_a))
        if init_actions is None:
            self._a_mat = torch.zeros(n_policies, hz_len, self.dim_a)
        else:
            assert init_actions.shape == (n_policies, hz_len, self.dim_a), "Initial actions shape mismatch."
            self._a_mat = init_actions.clone()
        self._a_mix = torch.ones(n_policies)
        self._params_log_space = params_log_space
        self._tf = None
        # forward() returns (costs, states, actions, omega, params_log_p) like the reference; states [M,S,N,H+1,ds] and
        # actions are tens of MB per call at demo sizes.  Callers that ignore them (the closed-loop drivers) set this False:
        # the rollout kernel then neither stores nor copies them (states / actions come back as None).
        self.return_rollouts = True
        if params_sampling is False or params_sampling is None or params_sampling == "none":
            self.n_params, self._sampling = 1, False
        elif params_sampling is True:
            self.n_params, self._sampling = params_samples, True
        elif isinstance(params_sampling, MerweScaledUTF):  # disco.py:124-131: sigma-point rollouts ("DISCO" case)
            assert self._params_log_space is False, "Distribution must not be on log space if using UTF."
            self.n_params, self._sampling = 1, True
            self._tf = params_sampling
        else:
            raise ValueError("Invalid value for 'params_sampling': {}".format(params_sampling))
        self.n_rollouts = self.n_params * self.n_actions * self.n_pol
        self._ctx = None
        self._ctx_key = None
        self._svmpc_cfg = {}
        self._device = kwargs.get("device", 0)
        self._seed = kwargs.get("seed", 0)
        # Reproducible runs: an object whose next_eps() / next_params() / next_ctrl_noise() return the next recorded draw (or None:
        # draw as usual) - policy noise [S,N,H,da] per SVGD step, dynamics samples [M,P] per sampling call, control-channel noise
        # [H, M*S*N, da] per rollout launch (Particle(deterministic=False), particle.py:145-148).  None (default): every draw is
        # fresh - policy / control noise from the device Philox stream, dynamics samples from params_dist.  The parity tests replay
        # the reference's own recorded draws through it (tests/helpers.py RecordedDraws).
        self.draw_source = None

    # ------------------------------------------------------------------ context management
    def _config(self, model, params_dist):
        if model.family not in ("pendulum", "particle", "skid_steer", "cartpole"):
            raise NotImplementedError("no rollout kernel family for %s" % type(model).__name__)
        chol = torch.linalg.cholesky(self.a_dist.covariance_matrix).diag()
        sigma = self.a_dist.covariance_matrix.diag().sqrt()  # svmpc.py:107-111
        cfg = dict(model=model.family, N=self.n_pol, S=self.n_actions, M=self._tf.pts if self._tf is not None else self.n_params, H=self.hz_len,
                   temperature=float(self.temp), ctrl_penalty=float(self._ctrl_penalty), alpha=1.0 / float(self.temp),
                   chol_a=chol.numpy(), sigma_a=sigma.numpy(), a_pre=self.a_pre.diag().numpy(),
                   a_cov=self.a_dist.covariance_matrix.numpy(),  # (a full matrix takes the off-diagonal path: disco.py:91-98)
                   min_a=self.min_a.numpy(), max_a=self.max_a.numpy(), device=self._device, seed=self._seed, dt=model.dt,
                   params_log_space=bool(self._params_log_space), sampling=self._sampling)
        if self._sampling:
            if self._tf is not None:
                self._scalar_event = False
            elif params_dist is not None:
                self._scalar_event = params_dist.event_shape == Empty
            elif getattr(self, "_scalar_event", None) is None:
                raise ValueError("params_sampling is on but no params_dist was given")
            cfg["uncertain_params"] = tuple(model.uncertain_params)
            cfg["params_scalar_event"] = self._scalar_event
        pd = model.params_dict
        for k in ("x_icr", "wheel_radius", "axial_distance"):  # SkidSteerRobot (skid_steer_robot.py:40-44)
            if k in pd:
                cfg[k] = float(pd[k])
        if model.family == "cartpole":  # CartPoleModel (cartpole.py:79-87); g and length follow below
            model.check_device_params()
            for k in ("f_mag", "mass_cart", "mass_pole", "mu_c", "mu_p"):
                cfg[k] = float(pd[k])
        for k in ("g", "mass", "length"):
            if k in pd:
                v = pd[k]
                cfg[k] = float(v)
                if k == "mass" and isinstance(v, torch.Tensor):
                    cfg["mass_0dim"] = True
        if model.family == "particle":
            cfg.update(max_speed=float(model._max_speed), max_accel=float(model._max_acc), can_crash=bool(model.can_crash),
                       with_obstacle=bool(model.with_obstacle), cell_size=float(model.map_cell_size or 0.1),
                       # particle.py:13-31, 145-153: control-channel noise and the control type reach the device rollouts
                       control_type=str(model.control_type), deterministic=bool(model.deterministic),
                       noise_std=tuple(float(v) for v in torch.as_tensor(model.dyn_std, dtype=torch.float).reshape(-1).expand(2)))
        cfg.update(recognise(model, self.inst_cost_fn, self.term_cost_fn))
        cfg.update(self._svmpc_cfg)
        nav = cost_grid_key(self.inst_cost_fn)
        if nav is not None:  # (part of the context key: a changed map rebuilds the context)
            cfg["nav_map"] = nav
        return cfg

    def _ensure_ctx(self, model, params_dist=None):
        cfg = self._config(model, params_dist)
        key = repr(sorted((k, np.asarray(v).tolist() if not isinstance(v, (str, bool, int, float, tuple)) else v) for k, v in cfg.items()))
        if self._ctx is not None and key == self._ctx_key:
            return self._ctx
        old = self._ctx
        state = None
        if old is not None:  # configuration changed: carry the state over
            state = dict(theta=old.get_theta(), prior=old.get_prior(), a_mat=old.get_a_mat(), a_seq=old.get_a_seq())
            old.close()
        grid = model.obst_map.map.astype(np.float32) if getattr(model, "obst_map", None) is not None else None
        if grid is None:  # the skid-steer model has no map of its own: a NavigationCost brings it
            grid = cost_grid(self.inst_cost_fn)
        self._ctx = Context(grid=grid, **{k: v for k, v in cfg.items() if k != "nav_map"})
        self._ctx_key = key
        if self._tf is not None:
            self._ctx.set_param_weights(self._tf.loc_weights.numpy())
            self._ctx.set_sigma_scale(self._tf.scale)
        if state is None:
            self._ctx.set_a_mat(self._a_mat.numpy())
            self._ctx.set_a_seq(self._a_seq.numpy())
        else:
            self._ctx.set_theta(state["theta"])
            self._ctx.set_prior(*state["prior"])
            self._ctx.set_a_mat(state["a_mat"])
            self._ctx.set_a_seq(state["a_seq"])
        return self._ctx

    def __deepcopy__(self, memo):
        new = copy.copy(self)
        memo[id(self)] = new
        for k, v in self.__dict__.items():
            if k == "_ctx":
                new._ctx = None if v is None else v.clone()
            elif k in ("inst_cost_fn", "term_cost_fn"):
                setattr(new, k, v)
            else:
                setattr(new, k, copy.deepcopy(v, memo))
        return new

    # ------------------------------------------------------------------ reference attributes backed by the device
    @property
    def a_mat(self):
        return torch.from_numpy(self._ctx.get_a_mat()) if self._ctx is not None else self._a_mat

    @a_mat.setter
    def a_mat(self, v):
        self._a_mat = torch.as_tensor(v, dtype=torch.float).detach().clone()
        if self._ctx is not None:
            self._ctx.set_a_mat(self._a_mat.numpy())

    @property
    def a_mix(self):
        return torch.from_numpy(self._ctx.get_a_mix()) if self._ctx is not None else self._a_mix

    @property
    def a_seq(self):
        return torch.from_numpy(self._ctx.get_a_seq()) if self._ctx is not None else self._a_seq

    @a_seq.setter
    def a_seq(self, v):
        self._a_seq = torch.as_tensor(v, dtype=torch.float).detach().clone()
        if self._ctx is not None:
            self._ctx.set_a_seq(self._a_seq.numpy())

    # ------------------------------------------------------------------ disco.py:348-394
    def _sigma_params(self, params_dist):
        """Sigma points of the parameter distribution (disco.py:238-251) and their weighted log-probability (288-291)."""
        try:
            cov, mean = params_dist.covariance_matrix, params_dist.mean
        except AttributeError:
            cov, mean = params_dist.variance.diag(), params_dist.mean
        sp = self._tf.compute_sigma_points(mean, cov).T.contiguous()  # [pts][P]
        lp = params_dist.log_prob(sp) @ self._tf.loc_weights
        return sp.reshape(1, self._tf.pts, -1).numpy(), lp.expand(self.n_actions, self.n_pol)

    def _sample_params(self, params_dist, n_sets=1):
        if not self._sampling:
            return None, None
        if self._tf is not None:
            sp, lp = self._sigma_params(params_dist)
            return np.repeat(sp, n_sets, axis=0), lp
        ps, lps = [], []
        for _ in range(n_sets):
            rec = self._recorded("params")  # recorded dynamics samples (draw_source), else a fresh draw
            p = params_dist.sample([self.n_params]) if rec is None else torch.as_tensor(rec, dtype=torch.float)
            lps.append(params_dist.log_prob(p))
            ps.append(p.reshape(self.n_params, -1))
        return torch.stack(ps).numpy(), lps[-1]

    def _recorded(self, kind):
        src = self.draw_source
        return None if src is None else getattr(src, "next_" + kind)()

    def _feed_ctrl_noise(self, ctx, n_sets=1):
        """Recorded control-channel noise for the next n_sets rollout launches, when the draw source has it."""
        if self.draw_source is None or not ctx.cfg.ctrl_noise:
            return
        rec = [self._recorded("ctrl_noise") for _ in range(n_sets)]
        if rec and rec[0] is not None:
            ctx.set_ctrl_noise(np.stack([np.asarray(r, np.float32) for r in rec]))

    def forward(self, state, model, params_dist=None, ext_actions=None, debug=False):
        ctx = self._ensure_ctx(model, params_dist)
        state = torch.as_tensor(state, dtype=torch.float).reshape(-1)
        params, params_log_p = self._sample_params(params_dist)
        acts = None if ext_actions is None else torch.as_tensor(ext_actions, dtype=torch.float).numpy()
        want = bool(self.return_rollouts)
        self._feed_ctrl_noise(ctx)
        costs, states, actions, omega = ctx.disco_forward(state.numpy(), acts, None if params is None else params[0],
                                                          want_states=want, want_actions=want)
        if not want:
            return torch.from_numpy(costs), None, None, torch.from_numpy(omega), params_log_p
        actions = torch.from_numpy(actions).unsqueeze(0).expand(self.n_params, -1, -1, -1, -1)
        return torch.from_numpy(costs), torch.from_numpy(states), actions, torch.from_numpy(omega), params_log_p

    def step(self, strategy="argmax", steps=1, ext_actions=None):  # disco.py:396-417
        if strategy not in ("argmax", "average", "external") or (strategy == "external" and ext_actions is None):
            raise ValueError("Invalid value for strategy.")
        if self._ctx is None:
            raise RuntimeError("step() before the first forward(): no rollouts have been evaluated yet")
        ext = None if ext_actions is None else torch.as_tensor(ext_actions, dtype=torch.float).numpy()
        try:
            return torch.from_numpy(self._ctx.disco_step(strategy, steps, ext))
        except L.DustError as e:
            raise ValueError(str(e))


class DiscoSimResult(collections.namedtuple("DiscoSimResult", "states actions costs loss status n_run a_seq")):
    """What BatchDISCO.simulate returns; `t0`: the periods the episode has run so far (simulate(resume=) goes on from there)"""


class BatchDISCO(MultiDISCO):
    """`n_envs` independent `MultiDISCO` controllers of one configuration - the deep copies the reference makes per episode
    (simulations.py:62, 78) - whose forward / step / tick are ONE kernel launch each, and whose closed-loop episodes are one launch per
    call (csrc/disco_batch.hpp).  Every environment has its own state, a_mat, a_seq, a_mix, noise stream (`seeds`, default seed + b) and
    parameter rows.  The constructor takes MultiDISCO's arguments behind `n_envs` and refuses what lies outside the kernel's box
    (N <= 64, S <= 1024, M <= 64, H d_a <= 128, a diagonal a_cov) before any device is touched.  `params_sampling=None` is the MPPI
    baseline of the reference's demo/pendulum_example.py, `params_sampling=MerweScaledUTF(...)` its DISCO case."""

    def __init__(self, n_envs, observation_space, action_space, hz_len, n_policies, action_samples, seeds=None, **kwargs):
        if not 1 <= int(n_envs) <= 65535:
            raise ValueError("n_envs = %d outside [1, 65535]" % int(n_envs))
        self.n_envs = int(n_envs)
        if seeds is not None and len(seeds) != self.n_envs:
            raise ValueError("seeds has %d entries for %d environments" % (len(seeds), self.n_envs))
        self._seeds = None if seeds is None else [int(v) for v in seeds]
        super().__init__(observation_space, action_space, hz_len, n_policies, action_samples, **kwargs)
        a_cov = self.a_dist.covariance_matrix
        if not torch.equal(a_cov, torch.diag(torch.diag(a_cov))):
            raise NotImplementedError("a batched MultiDISCO has a diagonal a_cov only (a full a_cov: lone MultiDISCO objects)")
        M = self._tf.pts if self._tf is not None else self.n_params
        for name, v, hi in (("n_policies", self.n_pol, 64), ("action_samples", self.n_actions, 1024),
                            ("sigma points" if self._tf is not None else "params_samples", M, 9 if self._tf is not None else 64),
                            ("hz_len * dim_a", self.hz_len * self.dim_a, 128)):
            if not 1 <= int(v) <= hi:
                raise ValueError("%s = %d outside [1, %d] for a batched MultiDISCO" % (name, int(v), hi))
        B = self.n_envs
        self._a_mat = self._a_mat[None].repeat(B, 1, 1, 1)
        self._a_seq = self._a_seq[None].repeat(B, 1, 1)
        self._a_mix = self._a_mix[None].repeat(B, 1)
        self._batch = None
        self._key = None

    # ------------------------------------------------------------------ device plumbing
    def _ensure_batch(self, model, params_dist=None):
        if self._tf is not None and model.family == "particle":
            raise NotImplementedError("a batched MultiDISCO has no sigma-point rollouts for Particle")
        pd0 = params_dist[0] if isinstance(params_dist, (list, tuple)) else params_dist
        cfg = self._config(model, pd0)
        key = repr(sorted((k, np.asarray(v).tolist() if not isinstance(v, (str, bool, int, float, tuple)) else v) for k, v in cfg.items()))
        if self._batch is not None and key == self._key:
            return self._batch
        carry = (self._a_mat.numpy(), self._a_seq.numpy())
        if self._batch is not None:  # configuration changed: carry every environment's plan over
            carry = (self._batch.get(L.DCB_A_MAT), self._batch.get(L.DCB_A_SEQ))
            self._batch.close()
            self._batch = None
        own_a_mat, own_a_seq = self._a_mat, self._a_seq
        self._a_mat, self._a_seq = own_a_mat[0], own_a_seq[0]  # (the prototype is a lone controller's context)
        try:
            proto = self._ensure_ctx(model, pd0)
        finally:
            self._a_mat, self._a_seq = own_a_mat, own_a_seq
        try:
            self._batch, self._key = proto.disco_batch(self.n_envs, self._seeds), key
        finally:
            proto.close()  # (the batch keeps its own copy)
            self._ctx = self._ctx_key = None
        self._batch.set(L.DCB_A_MAT, carry[0])
        self._batch.set(L.DCB_A_SEQ, carry[1])
        return self._batch

    def __deepcopy__(self, memo):
        new = copy.copy(self)
        memo[id(self)] = new
        for k, v in self.__dict__.items():
            if k == "_batch":
                new._batch = None if v is None else v.clone()
            elif k in ("inst_cost_fn", "term_cost_fn", "_ctx"):
                setattr(new, k, v)
            else:
                setattr(new, k, copy.deepcopy(v, memo))
        return new

    # ------------------------------------------------------------------ the plans, [B, ...]
    @property
    def a_mat(self):
        return torch.from_numpy(self._batch.get(L.DCB_A_MAT)) if self._batch is not None else self._a_mat

    @a_mat.setter
    def a_mat(self, v):
        self._a_mat = torch.as_tensor(v, dtype=torch.float).detach().clone().reshape(self.n_envs, self.n_pol, self.hz_len, self.dim_a)
        if self._batch is not None:
            self._batch.set(L.DCB_A_MAT, self._a_mat.numpy())

    @property
    def a_mix(self):
        return torch.from_numpy(self._batch.get(L.DCB_A_MIX)) if self._batch is not None else self._a_mix

    @property
    def a_seq(self):
        return torch.from_numpy(self._batch.get(L.DCB_A_SEQ)) if self._batch is not None else self._a_seq

    @a_seq.setter
    def a_seq(self, v):
        self._a_seq = torch.as_tensor(v, dtype=torch.float).detach().clone().reshape(self.n_envs, self.hz_len, self.dim_a)
        if self._batch is not None:
            self._batch.set(L.DCB_A_SEQ, self._a_seq.numpy())

    # ------------------------------------------------------------------ inputs
    def _states(self, states):
        return torch.as_tensor(states, dtype=torch.float).reshape(self.n_envs, -1).numpy()

    def _active(self, active):
        if active is None:
            return np.ones(self.n_envs, bool)
        on = np.asarray(torch.as_tensor(active).numpy() if isinstance(active, torch.Tensor) else active).reshape(-1) != 0
        if on.shape != (self.n_envs,):
            raise ValueError("active has %d entries for %d environments" % (on.size, self.n_envs))
        return on

    def _rows(self, params_dist, on, params=None):
        """[B, M, P]: the caller's rows, or what MultiDISCO.forward makes of `params_dist` (one distribution, or one per environment) -
        its sigma points, or one draw per active environment in environment order"""
        if params is not None:
            return np.asarray(torch.as_tensor(params, dtype=torch.float).numpy(), np.float32)
        if not self._sampling:
            return None
        pds = list(params_dist) if isinstance(params_dist, (list, tuple)) else [params_dist] * self.n_envs
        if len(pds) != self.n_envs:
            raise ValueError("%d parameter distributions for %d environments" % (len(pds), self.n_envs))
        rows = [np.asarray(self._sample_params(pds[b])[0][0], np.float32) if on[b] else None for b in range(self.n_envs)]
        shape = next(r for r in rows if r is not None).shape if on.any() else (self.n_params, 1)
        return np.stack([np.zeros(shape, np.float32) if r is None else r for r in rows])

    @staticmethod
    def _strategy(strategy, ext_actions, allow_external=True):
        if strategy not in ("argmax", "average", "external") or (strategy == "external" and (ext_actions is None or not allow_external)):
            raise ValueError("Invalid value for strategy.")

    def _steps(self, steps):
        if not 1 <= int(steps) <= self.hz_len:
            raise ValueError("steps = %d outside [1, hz_len = %d]" % (int(steps), self.hz_len))

    # ------------------------------------------------------------------ disco.py:348-417 for every environment
    def forward(self, states, model, params_dist=None, ext_actions=None, active=None, params=None):
        """states [B, ds]; ext_actions [B, S, N, H, da] or None (drawn on the device) -> (costs [B, S, N], omega [B, S, N])"""
        on = self._active(active)
        batch = self._ensure_batch(model, params_dist)
        acts = None if ext_actions is None else torch.as_tensor(ext_actions, dtype=torch.float).numpy()
        batch.forward(self._states(states), acts, self._rows(params_dist, on, params), None if active is None else on)
        return torch.from_numpy(batch.get(L.DCB_COSTS)), torch.from_numpy(batch.get(L.DCB_OMEGA))

    def step(self, strategy="argmax", steps=1, ext_actions=None, active=None):
        """-> next_actions [B, steps, da]; ext_actions [B, H, da] with "external"; the rows of inactive environments are NaN"""
        self._strategy(strategy, ext_actions)
        self._steps(steps)
        on = self._active(active)
        if self._batch is None:
            raise RuntimeError("step() before the first forward(): no rollouts have been evaluated yet")
        ext = None if ext_actions is None else torch.as_tensor(ext_actions, dtype=torch.float).numpy()
        return torch.from_numpy(self._batch.step(strategy, int(steps), ext, None if active is None else on))

    def tick(self, states, model, params_dist=None, strategy="argmax", steps=1, ext_actions=None, actions=None, active=None, params=None):
        """forward + step of every active environment in ONE launch -> next_actions [B, steps, da].  actions: recorded
        [B, S, N, H, da] (forward's ext_actions); ext_actions: step's rows [B, H, da]"""
        self._strategy(strategy, ext_actions)
        self._steps(steps)
        on = self._active(active)
        batch = self._ensure_batch(model, params_dist)
        acts = None if actions is None else torch.as_tensor(actions, dtype=torch.float).numpy()
        ext = None if ext_actions is None else torch.as_tensor(ext_actions, dtype=torch.float).numpy()
        return torch.from_numpy(batch.tick(self._states(states), strategy, int(steps), acts, self._rows(params_dist, on, params), ext,
                                           None if active is None else on))

    # ------------------------------------------------------------------ simulations.py:104-130, 217-260, the use_svmpc=False branch
    def _episode_inputs(self, model, params_dist, n_periods, strategy, plant_params, active, params):
        self._strategy(strategy, None, allow_external=False)
        T = int(n_periods)
        if not 1 <= T <= 4096:
            raise ValueError("n_periods = %d outside [1, 4096]: one launch runs one episode piece, split a longer one" % T)
        on = self._active(active)
        P = len(model.uncertain_params or ()) if self._sampling else 0
        if plant_params is not None:
            plant_params = np.asarray(torch.as_tensor(plant_params, dtype=torch.float).numpy(), np.float32)
            if P == 0 or plant_params.shape != (self.n_envs, P):
                raise ValueError("plant_params has shape %s, the plants read %s" % (plant_params.shape, (self.n_envs, P) if P else "none"))
        once = False
        if params is not None:
            rows = np.asarray(torch.as_tensor(params, dtype=torch.float).numpy(), np.float32)
            once = rows.ndim == 3
        elif not self._sampling:
            rows = None
        elif self._tf is not None:  # the sigma points of a fixed prior serve every period
            rows, once = self._rows(params_dist, on), True
        else:  # T successive draws of forward(), in period order
            rows = None
        return T, on, plant_params, rows, once

    def run_episodes(self, states, model, params_dist=None, n_periods=1, strategy="average", plant_params=None, active=None, params=None):
        """`n_periods` closed-loop periods - forward, step(strategy), the plant's step with that action under the environment's TRUE
        parameters `plant_params` [B, P] (None: the nominal model), without process noise - of every active environment in ONE launch.
        Dynamics rows: `params` [T, B, M, P] (or [B, M, P] for every period), else the sigma points of `params_dist`, else T successive
        draws as T calls of forward() make them.  -> (states [T, B, ds] after every step, actions [T, B, da], a_seq [B, H, da]); the
        rows of inactive environments are NaN."""
        T, on, plant_params, rows, once = self._episode_inputs(model, params_dist, n_periods, strategy, plant_params, active, params)
        batch = self._ensure_batch(model, params_dist)
        if rows is None and self._sampling:
            rows = np.stack([self._rows(params_dist, on) for _ in range(T)])
        xs, acts, a_seq = batch.episode(self._states(states), T, strategy, rows, plant_params, once, active=None if active is None else on)
        return torch.from_numpy(xs), torch.from_numpy(acts), torch.from_numpy(a_seq)

    def simulate(self, states, model, params_dist=None, n_periods=1, strategy="average", goal=None, goal_radius=None, stop_on_crash=False,
                 plant_params=None, active=None, params=None, resume=None, warm_up=0):
        """run_episodes() under the reference's episode rules, still ONE launch: the controller's instantaneous cost of every new state
        is recorded and summed in fp32 into `loss`; `stop_on_crash`: a new position on an occupied cell ends the environment with loss =
        inf, status 2; `goal` [ds] with `goal_radius` > 0: an environment within the radius ends with status 1.  This branch of the
        reference has no warm-up: `warm_up` must be 0.  `resume`: the result of a previous call - the episode goes on from its loss,
        status and period index.  -> DiscoSimResult(states, actions, costs [T, B], loss [B], status [B], n_run [B], a_seq) with the
        attribute t0; rows the call did not write are NaN (n_run: -1)."""
        if int(warm_up) != 0:
            raise ValueError("warm_up = %d: the MultiDISCO branch of the reference's loops has no warm-up" % int(warm_up))
        T, on, plant_params, rows, once = self._episode_inputs(model, params_dist, n_periods, strategy, plant_params, active, params)
        if (goal is None) != (goal_radius is None):
            raise ValueError("goal and goal_radius come together")
        rules = dict(stop_on_crash=bool(stop_on_crash))
        if goal is not None:
            goal = np.asarray(torch.as_tensor(goal, dtype=torch.float).numpy(), np.float32).reshape(-1)
            if goal.shape != (self.dim_s,) or not np.isfinite(goal).all():
                raise ValueError("goal has shape %s: [%d] finite entries" % (goal.shape, self.dim_s))
            if not (np.isfinite(float(goal_radius)) and float(goal_radius) > 0):
                raise ValueError("goal_radius must be finite and > 0")
            rules.update(goal=goal, goal_radius=float(goal_radius))
        if stop_on_crash:
            has_map = (model.family == "particle" and bool(model.with_obstacle)) or cost_grid_key(self.inst_cost_fn) is not None
            if not has_map:
                raise ValueError("stop_on_crash needs an occupancy map: Particle(with_obstacle=True) or a NavigationCost")
        loss = status = None
        if resume is not None:
            rules["t0"], loss, status = int(resume.t0), resume.loss.numpy(), resume.status.numpy()
            if loss.shape != (self.n_envs,) or status.shape != (self.n_envs,):
                raise ValueError("resume carries %d environments, the batch has %d" % (loss.size, self.n_envs))
        batch = self._ensure_batch(model, params_dist)
        if rows is None and self._sampling:
            rows = np.stack([self._rows(params_dist, on) for _ in range(T)])
        out = batch.episode(self._states(states), T, strategy, rows, plant_params, once, rules=rules, loss=loss, status=status,
                            active=None if active is None else on)
        res = DiscoSimResult(*(torch.from_numpy(np.ascontiguousarray(v)) for v in out))
        res.t0 = rules.get("t0", 0) + T
        return res
