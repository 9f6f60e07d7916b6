"""`AMPPI` with the reference's constructor, attributes and `update_actions` / `roll` signatures
(dust/controllers/amppi.py:6-260, dust/controllers/base.py:4-80): the single-policy information-theoretic MPC of Williams et al.
2017, one kernel launch per tick on the MI355X (csrc/amppi.hpp).

The controller owns one device context; `a_seq` lives there.  Parameter draws come from `model.sample_params(n)` on the host
(n = 1 or n_samples rows of a handful of columns: base.py:149-171), sigma points from `model.params_dist` through
`dust_amd.utils.utf.MerweScaledUTF`; everything else of the tick - noise, rollouts, costs, weights, the update - runs on the device.
`copy.deepcopy(controller)` clones the context."""
import collections
import copy

import numpy as np
import torch

from ..backend import Context
from ..costs import QuadraticCost, cost_grid, cost_grid_key, recognise
from ..inference.svmpc import _active
from ..utils.utf import MerweScaledUTF


class AMPPI:
    def __init__(self, observation_space, action_space, hz_len, n_samples, lambda_=1.0, a_cov=None, inst_cost_fn=None, term_cost_fn=None,
                 params_sampling="extended", init_actions=None, device=0, seed=0):
        self.hz_len = hz_len
        self.dim_s, self.dim_a = observation_space.dim, action_space.dim
        self.min_a, self.max_a = action_space.low, action_space.high
        # (the reference's `if not init_actions` raises on a tensor, base.py:34: None means zeros, a tensor is taken)
        if init_actions is None:
            self._a_seq = torch.zeros((hz_len, self.dim_a))
        else:
            self._a_seq = torch.as_tensor(init_actions, dtype=torch.float).detach().clone()
            assert self._a_seq.shape == (hz_len, self.dim_a), "Initial actions shape mismatch."
        if inst_cost_fn is None and term_cost_fn is None:
            raise ValueError("Specify at least one cost function")
        self.inst_cost_fn, self.term_cost_fn = inst_cost_fn, term_cost_fn
        self.n_samples = n_samples
        self.lambda_ = lambda_
        if a_cov is None:
            a_cov = torch.eye(self.dim_a)
        a_cov = torch.as_tensor(a_cov, dtype=torch.float)
        if not torch.equal(a_cov, torch.diag(torch.diag(a_cov))) and self.dim_a != 2:
            raise NotImplementedError("a full a_cov has a HIP kernel for dim_a = 2 (no CPU fallback)")
        self.a_dist = torch.distributions.multivariate_normal.MultivariateNormal(torch.zeros(self.dim_a), a_cov)
        self.a_pre = torch.inverse(a_cov)
        if not params_sampling or params_sampling == "none":
            self._sample_shape, self._tf = None, None
        elif params_sampling == "single":
            self._sample_shape, self._tf = 1, None
        elif params_sampling == "extended":
            self._sample_shape, self._tf = n_samples, None
        elif isinstance(params_sampling, MerweScaledUTF):
            self._sample_shape, self._tf = None, params_sampling
        else:
            raise ValueError("Invalid value for 'params_sampling': {}".format(params_sampling))
        self._params_sampling = params_sampling
        # update_actions returns (costs, states, acts, omega) like the reference; callers that ignore the trajectories set this False:
        # the kernel then stores no states and nothing but costs / omega is copied back (states / acts come back as None)
        self.return_rollouts = True
        self._ctx, self._ctx_key = None, None
        self._device, self._seed = device, seed

    @property
    def params_sampling(self):
        return self._params_sampling

    # ------------------------------------------------------------------ context management
    def _config(self, model):
        fam = getattr(model, "family", None)
        if fam not in ("pendulum", "particle", "skid_steer", "cartpole"):
            raise NotImplementedError("no AMPPI kernel family for %s" % type(model).__name__)
        if fam == "particle" and not model.deterministic:
            raise NotImplementedError("AMPPI runs Particle(deterministic=True): control-channel noise inside the tick is not implemented")
        if fam == "particle" and model.control_type != "acceleration":
            raise NotImplementedError("AMPPI runs Particle(control_type='acceleration')")
        owner = getattr(self.inst_cost_fn, "__self__", None)
        if isinstance(owner, QuadraticCost) and owner.w_ctrl is not None and bool((owner.w_ctrl != 0).any()):
            raise NotImplementedError("AMPPI's instantaneous cost sees no action (amppi.py:205); its control cost is the lambda term: "
                                      "QuadraticCost(w_ctrl=...) cannot be honoured")
        sampled = self._sample_shape is not None or self._tf is not None
        up = tuple(model.uncertain_params or ()) if sampled else ()
        if sampled and not up:
            raise ValueError("params_sampling is on but the model names no uncertain_params")
        if len(up) > 4:
            raise NotImplementedError("at most 4 uncertain parameters run on the device, got %d" % len(up))
        if self.hz_len * self.dim_a > 128:
            raise NotImplementedError("hz_len * dim_a = %d > 128 is not supported by the kernels" % (self.hz_len * self.dim_a))
        if not 1 <= self.n_samples <= 65536:
            raise NotImplementedError("n_samples = %d outside [1, 65536]" % self.n_samples)
        cov = self.a_dist.covariance_matrix
        cfg = dict(model=fam, N=1, S=self.n_samples, M=self._tf.pts if self._tf is not None else 1, H=self.hz_len,
                   temperature=float(self.lambda_), alpha=1.0 / float(self.lambda_), a_cov=cov.numpy(),  # (make_config factors a_cov itself)
                   min_a=torch.as_tensor(self.min_a, dtype=torch.float).reshape(-1).numpy(),
                   max_a=torch.as_tensor(self.max_a, dtype=torch.float).reshape(-1).numpy(),
                   device=self._device, seed=self._seed, dt=model.dt, sampling=sampled, uncertain_params=up)
        pd = model.params_dict
        for k in ("x_icr", "wheel_radius", "axial_distance"):
            if k in pd:
                cfg[k] = float(pd[k])
        if fam == "cartpole":
            for k in ("f_mag", "mass_cart", "mass_pole", "mu_c", "mu_p"):
                cfg[k] = float(pd[k])
        for k in ("g", "mass", "length"):
            if k in pd:
                cfg[k] = float(pd[k])
                if k == "mass" and isinstance(pd[k], torch.Tensor):
                    cfg["mass_0dim"] = True
        if fam == "particle":
            cfg.update(max_speed=float(model._max_speed), max_accel=float(model._max_acc), can_crash=bool(model.can_crash),
                       with_obstacle=bool(model.with_obstacle), cell_size=float(model.map_cell_size or 0.1), control_type="acceleration",
                       deterministic=True)
        cfg.update(recognise(model, self.inst_cost_fn, self.term_cost_fn))
        nav = cost_grid_key(self.inst_cost_fn)
        if nav is not None:  # (part of the context key: a changed map rebuilds the context)
            cfg["nav_map"] = nav
        return cfg

    def _new_ctx(self, model, cfg):
        """a fresh context of configuration cfg (`_config`), with the map and the sigma weights"""
        grid = model.obst_map.map.astype(np.float32) if getattr(model, "obst_map", None) is not None else None
        if grid is None:  # the skid-steer model has no map of its own: a NavigationCost brings it
            grid = cost_grid(self.inst_cost_fn)
        ctx = Context(grid=grid, **{k: v for k, v in cfg.items() if k != "nav_map"})
        if self._tf is not None:
            ctx.set_param_weights(self._tf.loc_weights.numpy())
        return ctx

    @staticmethod
    def _key(cfg):
        return repr(sorted((k, np.asarray(v).tolist() if not isinstance(v, (str, bool, int, float, tuple)) else v) for k, v in cfg.items()))

    def _ensure_ctx(self, model):
        cfg = self._config(model)
        key = self._key(cfg)
        if self._ctx is not None and key == self._ctx_key:
            return self._ctx
        a_seq = self.a_seq.numpy()
        if self._ctx is not None:
            self._ctx.close()
        self._ctx, self._ctx_key = self._new_ctx(model, cfg), key
        self._ctx.set_a_seq(a_seq)
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

    # ------------------------------------------------------------------ BaseController
    @property
    def a_seq(self):
        return torch.from_numpy(self._ctx.get_a_seq()) if self._ctx is not None else self._a_seq

    @a_seq.setter
    def a_seq(self, v):
        self._a_seq = torch.as_tensor(v, dtype=torch.float).detach().clone().reshape(self.hz_len, self.dim_a)
        if self._ctx is not None:
            self._ctx.set_a_seq(self._a_seq.numpy())

    def roll(self, steps=1):  # base.py:68-80
        if steps < 1:
            raise ValueError("roll(steps=%d): steps >= 1" % steps)
        if self._ctx is not None:
            self._ctx.amppi_roll(steps)
        else:
            self._a_seq = torch.cat((self._a_seq[steps:], torch.zeros(min(steps, self.hz_len), self.dim_a)), 0)

    # ------------------------------------------------------------------ amppi.py:227-260
    def _sigma_points(self, model):
        """amppi.py:164-175 -> [pts, P]"""
        pd = model.params_dist
        if pd is None:
            raise ValueError("a sigma-point controller reads model.params_dist: assign the parameter distribution to the model")
        try:
            cov, mean = pd.covariance_matrix, pd.mean
        except AttributeError:
            try:
                cov, mean = pd.variance.diag(), pd.mean
            except AttributeError:
                # (the reference's third form, `.a` / `.xs[i].S`, belongs to a mixture class it does not ship)
                raise NotImplementedError("model.params_dist has neither covariance_matrix nor variance")
        return self._tf.compute_sigma_points(mean, cov).T.contiguous().numpy()

    def update_actions(self, model, state, actions=None):
        """amppi.py:227-260 -> (costs [S], states [S pts, H + 1, ds], acts [S, H, da], omega [S]); `a_seq` is updated on the device.
        With `return_rollouts = False` nothing but costs and omega is stored or copied back: states and acts are None."""
        ctx = self._ensure_ctx(model)
        state = torch.as_tensor(state, dtype=torch.float).reshape(-1)
        acts = None if actions is None else torch.as_tensor(actions, dtype=torch.float).numpy()
        params, shared = None, False
        if self._tf is not None:
            params = self._sigma_points(model)
        elif self._sample_shape:
            params = model.dict_to_params(model.sample_params(self._sample_shape)).numpy()
            shared = self._params_sampling == "single"
        want = bool(self.return_rollouts)
        costs, omega, _, states, acts_out = ctx.amppi_update(state.numpy(), acts, params, shared_params=shared, want_states=want, want_actions=want)
        t = torch.from_numpy
        return t(costs), (t(states) if want else None), (t(acts_out) if want else None), t(omega)


class BatchAMPPI(AMPPI):
    """`n_envs` independent AMPPI controllers of one configuration - the deep copies the reference makes per episode
    (simulations.py) - ticking in ONE kernel launch (csrc/amppi.hpp amppi_batch_kernel).  Every environment has its own state, nominal
    sequence, noise stream (`seeds`, default seed + b) and parameter rows; environment b computes what an `AMPPI(seed=seeds[b])`
    computes on its inputs, bit for bit.  The constructor takes AMPPI's arguments behind `n_envs` and refuses what AMPPI refuses."""

    def __init__(self, n_envs, *args, seeds=None, **kw):
        super().__init__(*args, **kw)
        if not 1 <= int(n_envs) <= 65535:
            raise ValueError("n_envs = %d outside [1, 65535]" % int(n_envs))
        self.n_envs = int(n_envs)
        if seeds is not None and len(seeds) != self.n_envs:
            raise ValueError("seeds has %d entries for %d environments" % (len(seeds), self.n_envs))
        self._seeds = None if seeds is None else [int(v) for v in seeds]
        self._a_seq = self._a_seq[None].repeat(self.n_envs, 1, 1)  # [B, H, da]
        self._batch = None

    def _ensure_batch(self, model):
        cfg = self._config(model)
        key = self._key(cfg)
        if self._batch is not None and key == self._ctx_key:
            return self._batch
        a_seq = self.a_seq.numpy()
        if self._batch is not None:
            self._batch.close()
        proto = self._new_ctx(model, cfg)
        try:
            self._batch, self._ctx_key = proto.amppi_batch(self.n_envs, self._seeds), key
        finally:
            proto.close()  # (the batch keeps its own copy)
        self._batch.set_a_seq(a_seq)
        return self._batch

    def __deepcopy__(self, memo):
        new = copy.copy(self)
        memo[id(self)] = new
        for k, v in self.__dict__.items():
            if k == "_batch":
                new._batch = None if v is None else v.clone()
            elif k in ("inst_cost_fn", "term_cost_fn"):
                setattr(new, k, v)
            else:
                setattr(new, k, copy.deepcopy(v, memo))
        return new

    @property
    def a_seq(self):
        """[B, H, da]"""
        return torch.from_numpy(self._batch.get_a_seq()) if self._batch is not None else self._a_seq

    @a_seq.setter
    def a_seq(self, v):
        self._a_seq = torch.as_tensor(v, dtype=torch.float).detach().clone().reshape(self.n_envs, self.hz_len, self.dim_a)
        if self._batch is not None:
            self._batch.set_a_seq(self._a_seq.numpy())

    def _active(self, active):
        return _active(active, self.n_envs)

    def roll(self, steps=1, active=None):
        if steps < 1:
            raise ValueError("roll(steps=%d): steps >= 1" % steps)
        if self._batch is not None:
            self._batch.roll(steps, active)
            return
        on = torch.from_numpy(self._active(active))
        rolled = torch.cat((self._a_seq[:, steps:], torch.zeros(self.n_envs, min(steps, self.hz_len), self.dim_a)), 1)
        self._a_seq = torch.where(on.view(-1, 1, 1), rolled, self._a_seq)

    def update_actions(self, model, states, actions=None, active=None, params=None):
        """One tick of every active environment -> (costs [B, S], None, acts [B, S, H, da], omega [B, S]); the rows of inactive
        environments are NaN, and `acts` is None with `return_rollouts = False`.  states [B, ds]; actions [B, S, H, da] or None (drawn
        on the device); params [B, rows, P] overrides the class's own parameter draws - one parameter distribution per environment;
        without it the class makes the draws AMPPI makes, once per active environment in environment order."""
        batch = self._ensure_batch(model)
        B = self.n_envs
        states = torch.as_tensor(states, dtype=torch.float).reshape(B, -1)
        acts = None if actions is None else torch.as_tensor(actions, dtype=torch.float).numpy()
        on = self._active(active)
        shared = self._params_sampling == "single"
        if params is not None:
            params = torch.as_tensor(params, dtype=torch.float).numpy()
        elif self._tf is not None:
            params = np.repeat(self._sigma_points(model)[None], B, 0)
        elif self._sample_shape:
            rows = [model.dict_to_params(model.sample_params(self._sample_shape)).numpy() if on[b] else None for b in range(B)]
            shape = next((r.shape for r in rows if r is not None), None)
            if shape is not None:
                params = np.stack([r if r is not None else np.zeros(shape, np.float32) for r in rows])
        want = bool(self.return_rollouts)
        if params is None and (self._tf is not None or self._sample_shape) and not on.any():  # nobody ticks: nothing to launch
            nan = lambda *sh: torch.full(sh, float("nan"))
            return (nan(B, self.n_samples), None, nan(B, self.n_samples, self.hz_len, self.dim_a) if want else None, nan(B, self.n_samples))
        costs, omega, _, acts_out = batch.update(states.numpy(), acts, params, shared_params=shared and params is not None,
                                                 active=None if active is None else on, want_actions=want)
        t = torch.from_numpy
        return t(costs), None, (t(acts_out) if want else None), t(omega)

    def run_episodes(self, model, states, n_periods, plant_params=None, active=None, roll_steps=1):
        """`n_periods` closed-loop periods of every active environment with the plants on the device (dust_amppi_batch_episode): per
        period update_actions with device-drawn noise, the plant's step with the first action of the updated sequence - the model's
        own step under the environment's TRUE parameters `plant_params` [B, P] (the columns of the controller's parameter rows; None:
        the nominal model), without process noise - and roll(roll_steps); the host does not come between two periods.  states [B, ds]:
        where the episodes start.  The parameter rows are the draws `n_periods` calls of update_actions would make, in the same order:
        under one torch.manual_seed the call consumes the torch stream exactly as they do.
        -> (states [T, B, ds] after every step, actions [T, B, da], costs [T, B, S], omega [T, B, S]); the rows of inactive
        environments are NaN."""
        T, B = int(n_periods), self.n_envs
        if not 1 <= T <= 4096:
            raise ValueError("n_periods = %d outside [1, 4096]: one call runs one episode piece, split a longer one" % T)
        if roll_steps < 1:
            raise ValueError("roll(steps=%d): steps >= 1" % roll_steps)
        on = self._active(active)
        sampled = self._tf is not None or bool(self._sample_shape)
        P = len(getattr(model, "uncertain_params", None) or ()) if sampled else 0
        if plant_params is not None:
            plant_params = np.asarray(torch.as_tensor(plant_params, dtype=torch.float).numpy(), np.float32)
            if P == 0 or plant_params.shape != (B, P):
                raise ValueError("plant_params has shape %s, the plants read %s" % (plant_params.shape, (B, P) if P else "none"))
        states = torch.as_tensor(states, dtype=torch.float).reshape(B, -1)
        batch = self._ensure_batch(model)
        params = None
        if self._tf is not None and on.any():
            params = np.stack([np.repeat(self._sigma_points(model)[None], B, 0) for _ in range(T)])
        elif self._sample_shape and on.any():
            per = []
            for _ in range(T):  # (update_actions' draws: once per active environment, in environment order)
                rows = [model.dict_to_params(model.sample_params(self._sample_shape)).numpy() if on[b] else None for b in range(B)]
                shape = next(r.shape for r in rows if r is not None)
                per.append(np.stack([r if r is not None else np.zeros(shape, np.float32) for r in rows]))
            params = np.stack(per)
        if params is None and sampled:  # nobody ticks: nothing to launch
            nan = lambda *sh: torch.full(sh, float("nan"))
            return nan(T, B, states.shape[1]), nan(T, B, self.dim_a), nan(T, B, self.n_samples), nan(T, B, self.n_samples)
        xs, acts, costs, omega, _ = batch.episode(states.numpy(), T, params, shared_params=self._params_sampling == "single" and params is not None,
                                                  plant_params=plant_params, active=None if active is None else on, roll_steps=roll_steps)
        t = torch.from_numpy
        return t(xs), t(acts), t(costs), t(omega)

    # -- run_particle_episode's use_svmpc=False branch / run_pendulum_simulation's AMPPI loop (simulations.py:217-260, 124-160) for every
    # environment: the episode under the reference's rules - the accumulated cost, crash and goal; this branch has no warm-up
    def simulate(self, model, states, n_periods, goal=None, goal_radius=None, stop_on_crash=False, plant_params=None, active=None, roll_steps=1,
                 resume=None, params=None):
        """run_episodes() under the reference's episode rules (dust_amppi_batch_simulate), still one launch per period and no host between
        two periods: the controller's instantaneous cost of every new state is recorded and summed in fp32 into `loss`; `stop_on_crash`: a
        new position on an occupied cell of the model's (or the navigation cost's) map ends the environment with loss = inf, status 2;
        `goal` [ds] with `goal_radius` > 0: an environment within the radius ends with status 1.  `resume`: the result of a previous call
        - the episode goes on from its loss, status and period index (a changed plant, such as the reference's load at steps // 4, is two
        calls).  The parameter rows are drawn as run_episodes() draws them - under one torch.manual_seed the call consumes the torch
        stream as `n_periods` calls of update_actions with the same `active` do - unless `params` [T, B, rows, P] overrides them.
        -> AmppiSimResult(states [T, B, ds], actions [T, B, da], costs [T, B, S], omega [T, B, S], inst_costs [T, B], loss [B], status
        [B], n_run [B], a_seq [B, H, da] of every environment's last period before its roll) with the attribute t0 (the periods the
        episode has run); rows the call did not write - past n_run[b], inactive environments - are NaN (n_run: -1)."""
        T, B = int(n_periods), self.n_envs
        if not 1 <= T <= 4096:
            raise ValueError("n_periods = %d outside [1, 4096]: one call runs one episode piece, split a longer one" % T)
        if roll_steps < 1:
            raise ValueError("roll(steps=%d): steps >= 1" % roll_steps)
        on = self._active(active)
        sampled = self._tf is not None or bool(self._sample_shape)
        P = len(getattr(model, "uncertain_params", None) or ()) if sampled else 0
        if plant_params is not None:
            plant_params = np.asarray(torch.as_tensor(plant_params, dtype=torch.float).numpy(), np.float32)
            if P == 0 or plant_params.shape != (B, P):
                raise ValueError("plant_params has shape %s, the plants read %s" % (plant_params.shape, (B, P) if P else "none"))
        goal, goal_radius = _sim_goal(goal, goal_radius, self.dim_s)
        if stop_on_crash:
            has_map = (getattr(model, "family", None) == "particle" and bool(model.with_obstacle)) or cost_grid_key(self.inst_cost_fn) is not None
            if not has_map:
                raise ValueError("stop_on_crash needs an occupancy map: Particle(with_obstacle=True) or a NavigationCost")
        t0, loss, status = _sim_resume(resume, B)
        states = torch.as_tensor(states, dtype=torch.float).reshape(B, -1)
        batch = self._ensure_batch(model)
        if params is not None:
            params = np.asarray(torch.as_tensor(params, dtype=torch.float).numpy(), np.float32)
        elif self._tf is not None and on.any():
            params = np.stack([np.repeat(self._sigma_points(model)[None], B, 0) for _ in range(T)])
        elif self._sample_shape and on.any():
            per = []
            for _ in range(T):  # (update_actions' draws: once per active environment, in environment order)
                rows = [model.dict_to_params(model.sample_params(self._sample_shape)).numpy() if on[b] else None for b in range(B)]
                shape = next(r.shape for r in rows if r is not None)
                per.append(np.stack([r if r is not None else np.zeros(shape, np.float32) for r in rows]))
            params = np.stack(per)
        if params is None and sampled:  # nobody ticks: nothing to launch
            nan = lambda *sh: torch.full(sh, float("nan"))
            S = self.n_samples
            res = AmppiSimResult(nan(T, B, states.shape[1]), nan(T, B, self.dim_a), nan(T, B, S), nan(T, B, S), nan(T, B),
                                 torch.zeros(B) if loss is None else torch.from_numpy(np.array(loss, np.float32)),
                                 torch.zeros(B, dtype=torch.int32) if status is None else torch.from_numpy(np.array(status, np.int32)),
                                 torch.full((B,), -1, dtype=torch.int32), nan(B, self.hz_len, self.dim_a))
            res.t0 = t0 + T
            return res
        out = batch.simulate(states.numpy(), T, params, shared_params=self._params_sampling == "single" and params is not None,
                             plant_params=plant_params, t0=t0, goal=goal, goal_radius=goal_radius, stop_on_crash=stop_on_crash, loss=loss,
                             status=status, active=None if active is None else on, roll_steps=roll_steps)
        res = AmppiSimResult(*(torch.from_numpy(np.ascontiguousarray(v)) for v in out))
        res.t0 = t0 + T
        return res


def _sim_goal(goal, goal_radius, ds):
    """the goal rule's arguments as the library reads them (both None: no goal rule); refused on the host what needs no device"""
    if (goal is None) != (goal_radius is None):
        raise ValueError("goal and goal_radius come together")
    if goal is None:
        return None, None
    goal = np.asarray(torch.as_tensor(goal, dtype=torch.float).numpy(), np.float32).reshape(-1)
    if goal.shape != (ds,) or not np.isfinite(goal).all():
        raise ValueError("goal has shape %s: [%d] finite entries" % (goal.shape, ds))
    if not (np.isfinite(float(goal_radius)) and float(goal_radius) > 0):
        raise ValueError("goal_radius must be finite and > 0")
    return goal, float(goal_radius)


def _sim_resume(resume, B):
    """(t0, loss, status) a call goes on from: the result of a previous simulate(), or the episode's start"""
    if resume is None:
        return 0, None, None
    loss, status = resume.loss.numpy(), resume.status.numpy()
    if loss.shape != (B,) or status.shape != (B,):
        raise ValueError("resume carries %d environments, the batch has %d" % (loss.size, B))
    return int(resume.t0), loss, status


class AmppiSimResult(collections.namedtuple("AmppiSimResult", "states actions costs omega inst_costs loss status n_run a_seq")):
    """What BatchAMPPI.simulate returns; `t0`: the periods the episode has run so far (simulate(resume=) goes on from there)"""
    t0 = 0


class DualAmppiSimResult(collections.namedtuple("DualAmppiSimResult", "states actions costs omega bw inst_costs loss status n_run a_seq")):
    """What BatchDualAMPPI.simulate returns; `t0` as AmppiSimResult's"""
    t0 = 0
