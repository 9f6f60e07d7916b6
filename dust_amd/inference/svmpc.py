"""`SVMPC` with the reference's constructor and methods (dust/inference/svmpc.py:14-200, svgd.py:109-125)."""
import collections

import numpy as np
import torch

from ..kernels import kernel_config
from ..optim import check_optimizer, group_options, optimizer_config


def _configure(oc, likelihood, cov, weighted_prior, roll_strategy, kernel_cfg):
    """The optimiser's options `oc` (optimizer_config) and SVMPC's own into the controller's configuration; plain SGD / Adam keep
    dust_config's own fields."""
    opt = dict(optimizer="Adam" if oc["kind"] == "Adam" else "SGD", lr=oc["lr"], optim=oc)
    if oc["kind"] == "Adam":
        opt["adam"] = (oc["beta1"], oc["beta2"], oc["eps"])
    likelihood.controller._svmpc_cfg.update(opt, likelihood=likelihood.kind, alpha=float(likelihood.alpha), weighted_prior=bool(weighted_prior),
                                            roll_strategy=roll_strategy, sigma_p=cov.diag().sqrt().numpy(), p_cov=cov.detach().numpy().copy(),
                                            **kernel_cfg)


def _active(active, n_envs):
    """the active mask as [n_envs] bools (None: everybody)"""
    if active is None:
        return np.ones(n_envs, bool)
    a = np.asarray(active).reshape(-1) != 0
    if a.shape != (n_envs,):
        raise ValueError("active has %d entries for %d environments" % (a.size, n_envs))
    return a


class SVMPC:
    def __init__(self, init_particles, prior, likelihood, roll_strategy="repeat", weighted_prior=False, kernel=None, bw_scale=1.0,
                 n_particles=None, n_steps=100, optimizer_class=torch.optim.Adam, **opt_args):
        self.likelihood = likelihood
        self.kernel, self.bw_scale = kernel, bw_scale
        self.n_particles = n_particles if n_particles is not None else init_particles.shape[0]
        self.n_steps = n_steps
        self.optimizer_class, self.opt_args = optimizer_class, opt_args
        self.w_prior, self.roll_strategy = weighted_prior, roll_strategy
        if roll_strategy not in ("repeat", "mean", "resample"):
            raise ValueError("{} is an invalid roll strategy.".format(roll_strategy))
        self._optim = optimizer_config(optimizer_class, opt_args)  # every option reaches the device or raises (dust_amd/optim.py)
        comp = prior.component_distribution.base_dist
        cov = comp.covariance_matrix
        cov = cov.reshape(-1, cov.shape[-2], cov.shape[-1])[0]
        if not torch.equal(cov, torch.diag(torch.diag(cov))) and cov.shape[-1] != 2:
            raise NotImplementedError("a full prior covariance has a HIP kernel for dim_a = 2")
        _configure(self._optim, likelihood, cov, weighted_prior, roll_strategy, kernel_config(kernel))
        self._theta0 = torch.as_tensor(init_particles, dtype=torch.float).detach().clone()
        self._prior0 = (comp.loc.detach().clone(), prior.mixture_distribution.probs.detach().clone())
        self._uploaded = False
        self._prior_obj, self._prior_cov = prior, cov
        self._prior_stale = False
        # attribute compatibility (simulations.py never touches it): torch's optimiser object over a placeholder - the optimiser
        # STATE lives on the device and restarts at every roll, as torch's does when roll() swaps the parameter tensor
        self.optimizer = optimizer_class(params=[torch.zeros(1, requires_grad=True)], **opt_args)
        self._opt_group = group_options(self.optimizer)  # (what the device runs: check_optimizer refuses later edits of the group)

    # -- device plumbing
    def _ctx(self, params_dist=None):
        ctrl = self.likelihood.controller
        ctx = ctrl._ensure_ctx(self.likelihood.model, params_dist)
        if not self._uploaded:
            ctx.set_theta(self._theta0.numpy())
            ctx.set_prior(self._prior0[0].numpy(), self._prior0[1].numpy())
            self._uploaded = True
        return ctx

    def __deepcopy__(self, memo):
        import copy

        new = copy.copy(self)
        memo[id(self)] = new
        for k, v in self.__dict__.items():
            setattr(new, k, v if k in ("kernel", "optimizer_class") else copy.deepcopy(v, memo))
        if self._uploaded:  # the cloned controller context already carries theta / prior
            new._uploaded = True
        return new

    @property
    def theta(self):
        return torch.from_numpy(self._ctx().get_theta()) if self._uploaded else self._theta0

    @theta.setter
    def theta(self, v):
        self._theta0 = torch.as_tensor(v, dtype=torch.float).detach().clone()
        if self._uploaded:
            self._ctx().set_theta(self._theta0.numpy())

    @property
    def prior(self):
        """The GMM in force (svmpc.py:160-170): after a forward() / update_prior() its means are the current particles."""
        if self._prior_stale and self._uploaded:
            from .svgd import get_gmm

            means, probs = self._ctx().get_prior()
            self._prior_obj = get_gmm(torch.from_numpy(means), torch.from_numpy(probs), self._prior_cov)
            self._prior_stale = False
        return self._prior_obj

    @prior.setter
    def prior(self, p):
        self._prior_obj = p
        comp = p.component_distribution.base_dist
        self._prior_stale = False
        if self._uploaded:
            self._ctx().set_prior(comp.loc.detach().numpy(), p.mixture_distribution.probs.detach().numpy())
        else:
            self._prior0 = (comp.loc.detach().clone(), p.mixture_distribution.probs.detach().clone())

    # -- svmpc.py:32-85
    def phi(self, log_p, bw=None, sigma=None):
        ctx = self._ctx()
        _, costs, actions = log_p(self.theta)
        phi, _, _ = ctx.svmpc_phi(torch.as_tensor(costs).numpy(), torch.as_tensor(actions).numpy())
        return torch.from_numpy(phi)

    def _state(self, state):
        return torch.as_tensor(state, dtype=torch.float).reshape(-1).numpy()

    # -- svmpc.py:87-126
    def step(self, state, params_dist, bw=None, sigma=None, eps=None):
        self.optimize(state, params_dist, n_steps=1, eps=None if eps is None else np.asarray(eps, np.float32)[None])

    def optimize(self, state, params_dist, bw=None, n_steps=None, debug=False, eps=None):
        """`bw` is accepted and ignored, as in the reference (dead value on both kernel branches)."""
        check_optimizer(self.optimizer, self._opt_group)  # (an LR scheduler / a second param group on `self.optimizer` would not reach the device)
        ctx = self._ctx(params_dist)
        ctrl = self.likelihood.controller
        n_steps = self.n_steps if n_steps is None else n_steps
        if eps is None and ctrl.draw_source is not None:  # recorded draws (MultiDISCO.draw_source), e.g. of a reference run
            rec = [ctrl._recorded("eps") for _ in range(n_steps)]
            if rec and rec[0] is not None:
                eps = np.stack([np.asarray(r, np.float32) for r in rec])
        params, lp = ctrl._sample_params(params_dist, n_steps)
        self.likelihood.params_log_p = lp
        ctrl._feed_ctrl_noise(ctx, n_steps)
        ctx.svmpc_optimize(self._state(state), n_steps, eps, params)

    # -- svmpc.py:128-200
    def _resample(self, ctx):
        if self.roll_strategy != "resample":
            return None
        # svmpc.py:148-150: the last action of a fresh prior sample per particle (torch's RNG, as in the reference)
        return self.prior.sample([self.n_particles])[..., -1, :].reshape(self.n_particles, -1).numpy()

    def get_weights(self, state, params_dist, fast_pred=True):
        ctx = self._ctx(params_dist)
        if not fast_pred:
            params, _ = self.likelihood.controller._sample_params(params_dist)
            ctx.likelihood_sample(self._state(state), None, None if params is None else params[0])
        return torch.from_numpy(ctx.svmpc_get_weights())

    def roll(self, steps=-1, strategy="repeat"):
        ctx = self._ctx()
        last = None
        if strategy == "resample":
            last = self.prior.sample([self.n_particles])[..., -1, :].reshape(self.n_particles, -1).numpy()
        ctx.svmpc_roll(steps, strategy, last)

    def update_prior(self, weights=None):
        self._ctx().svmpc_update_prior(None if weights is None else torch.as_tensor(weights, dtype=torch.float).numpy())
        self._prior_stale = True

    def forward(self, state, params_dist, steps=-1, fast_pred=True):
        ctx = self._ctx(params_dist)
        if not fast_pred:
            params, _ = self.likelihood.controller._sample_params(params_dist)
            ctx.likelihood_sample(self._state(state), None, None if params is None else params[0])
        a_seq, pw = ctx.svmpc_forward_ex(steps, self._resample(ctx))
        self._prior_stale = True
        return torch.from_numpy(a_seq), torch.from_numpy(pw)

    def tick(self, state, params_dist, n_steps=None, eps=None):
        """optimize + forward enqueued back to back (dust_svmpc_tick)."""
        check_optimizer(self.optimizer, self._opt_group)
        ctx = self._ctx(params_dist)
        n_steps = self.n_steps if n_steps is None else n_steps
        params, _ = self.likelihood.controller._sample_params(params_dist, n_steps)
        if self.roll_strategy == "resample":  # the last row is drawn on the host between the two halves
            ctx.svmpc_optimize(self._state(state), n_steps, eps, params)
            a_seq, pw = ctx.svmpc_forward_ex(-1, self._resample(ctx))
        else:
            a_seq, pw = ctx.svmpc_tick(self._state(state), n_steps, eps, params)
        self._prior_stale = True
        return torch.from_numpy(a_seq), torch.from_numpy(pw)


class BatchSVMPC:
    """`n_envs` independent `SVMPC` controllers of one configuration - the deep copies the reference makes per episode
    (simulations.py:62,78) - whose optimize / forward / tick are ONE kernel launch each (csrc/svmpc_batch.hpp svmpc_batch_kernel).
    Every environment has its own state, particles, prior, a_mat, optimiser state, noise stream (`seeds`, default seed + b) and
    dynamics samples.  The constructor takes SVMPC's arguments behind `n_envs` and refuses what lies outside the kernel's box
    (K1 / IMQ kernel, N <= 64, S <= 1024, M <= 64, H d_a <= 128, ctrl_penalty = 1, diagonal covariances, no sigma points, roll
    'repeat' / 'mean') before any device is touched.  Every model family's cost runs in the batch, the skid-steer robot's
    `NavigationCost` among them (svmpc_skid_nav_batch_kernel): its one occupancy map serves all `n_envs` environments.
    `set_hyper` gives every environment its own lr, alpha, temperature, prior_sigma, ctrl_sigma and weighted_prior (svmpc_sweep_kernel):
    a hyper-parameter sweep is then one `run_episodes` call."""

    def __init__(self, n_envs, init_particles, prior, likelihood, roll_strategy="repeat", weighted_prior=False, kernel=None, bw_scale=1.0,
                 n_particles=None, n_steps=100, optimizer_class=torch.optim.Adam, seeds=None, **opt_args):
        if not 1 <= int(n_envs) <= 65535:
            raise ValueError("n_envs = %d outside [1, 65535]" % int(n_envs))
        self.n_envs = int(n_envs)
        if seeds is not None and len(seeds) != self.n_envs:
            raise ValueError("seeds has %d entries for %d environments" % (len(seeds), self.n_envs))
        self._seeds = None if seeds is None else [int(v) for v in seeds]
        if roll_strategy not in ("repeat", "mean", "resample"):
            raise ValueError("{} is an invalid roll strategy.".format(roll_strategy))
        if roll_strategy == "resample":
            raise NotImplementedError("a batched SVMPC tick rolls with 'repeat' or 'mean': 'resample' draws on the host between the two halves")
        kc = kernel_config(kernel)
        if kc["kernel"] not in ("K1", "IMQ"):
            raise NotImplementedError("a batched SVMPC tick has the K1 (RBFKernel) and the IMQ kernel; %s runs on lone SVMPC objects" % kc["kernel"])
        ctrl = likelihood.controller
        if ctrl._tf is not None:
            raise NotImplementedError("a batched SVMPC tick has no sigma-point rollouts (params_sampling=MerweScaledUTF)")
        if float(ctrl._ctrl_penalty) != 1.0:
            raise NotImplementedError("a batched SVMPC tick has no control-cost term: ctrl_penalty = 1 (got %g)" % float(ctrl._ctrl_penalty))
        a_cov = ctrl.a_dist.covariance_matrix
        comp = prior.component_distribution.base_dist
        cov = comp.covariance_matrix
        cov = cov.reshape(-1, cov.shape[-2], cov.shape[-1])[0]
        if not torch.equal(a_cov, torch.diag(torch.diag(a_cov))) or not torch.equal(cov, torch.diag(torch.diag(cov))):
            raise NotImplementedError("a batched SVMPC tick has diagonal covariances only (a full a_cov / prior covariance: lone SVMPC objects)")
        init_particles = torch.as_tensor(init_particles, dtype=torch.float).detach().clone()
        N = int(init_particles.shape[-3])
        for name, v, hi in (("n_particles", N, 64), ("action_samples", ctrl.n_actions, 1024), ("params_samples", ctrl.n_params, 64),
                            ("hz_len * dim_a", ctrl.hz_len * ctrl.dim_a, 128)):
            if not 1 <= int(v) <= hi:
                raise ValueError("%s = %d outside [1, %d] for a batched SVMPC tick" % (name, int(v), hi))
        if N != ctrl.n_pol:
            raise ValueError("init_particles has %d particles, the controller has n_policies = %d" % (N, ctrl.n_pol))
        self.likelihood = likelihood
        self.kernel, self.bw_scale = kernel, bw_scale
        self.n_particles = n_particles if n_particles is not None else N
        self.n_steps = n_steps
        self.optimizer_class, self.opt_args = optimizer_class, opt_args
        self.w_prior, self.roll_strategy = weighted_prior, roll_strategy
        self._optim = optimizer_config(optimizer_class, opt_args)
        _configure(self._optim, likelihood, cov, weighted_prior, roll_strategy, kc)
        B = self.n_envs
        shape = (N, ctrl.hz_len, ctrl.dim_a)
        self._theta0 = (init_particles if init_particles.ndim == 4 else init_particles[None].repeat(B, 1, 1, 1)).reshape((B,) + shape).clone()
        self._prior0 = (comp.loc.detach().clone().reshape(shape), prior.mixture_distribution.probs.detach().clone().reshape(N))
        self._prior_cov = cov
        self._batch = None
        self._key = None
        self._hyper = None  # set_hyper(): per-environment rows (a dict of arrays), kept here until - and whenever - a batch is built
        self._history = (False, False)  # set_history(): (theta, filter), kept here likewise
        self.optimizer = optimizer_class(params=[torch.zeros(1, requires_grad=True)], **opt_args)
        self._opt_group = group_options(self.optimizer)

    # -- device plumbing
    def _ensure_batch(self, params_dist=None):
        ctrl = self.likelihood.controller
        cfg = ctrl._config(self.likelihood.model, params_dist)
        key = repr(sorted((k, np.asarray(v).tolist() if not isinstance(v, (str, bool, int, float, tuple)) else v) for k, v in cfg.items()))
        if self._batch is not None and key == self._key:
            return self._batch
        from .. import _lib as L

        carry = None
        if self._batch is not None:  # configuration changed: carry every environment's state over
            old = self._batch
            carry = [old.get(w) for w in (L.SVB_THETA, L.SVB_PRIOR_MEANS, L.SVB_PRIOR_MIX, L.SVB_A_MAT)]
            old.close()
            self._batch = None
        proto = ctrl._ensure_ctx(self.likelihood.model, params_dist)
        try:
            proto.set_theta(self._theta0[0].numpy())
            proto.set_prior(self._prior0[0].numpy(), self._prior0[1].numpy())
            self._batch, self._key = proto.svmpc_batch(self.n_envs, self._seeds), key
        finally:
            proto.close()  # (the batch keeps its own copy)
            ctrl._ctx = ctrl._ctx_key = None
        if carry is not None:
            for w, v in zip((L.SVB_THETA, L.SVB_PRIOR_MEANS, L.SVB_PRIOR_MIX, L.SVB_A_MAT), carry):
                self._batch.set(w, v)
        elif not all(torch.equal(self._theta0[b], self._theta0[0]) for b in range(1, self.n_envs)):
            self._batch.set(L.SVB_THETA, self._theta0.numpy())
        if self._hyper is not None:  # the per-environment rows belong to this object: a new or a rebuilt batch gets them again
            self._batch.set_hyper(self._hyper)
        if any(self._history):
            self._batch.set_history(*self._history)
        return self._batch

    # -- per-environment hyper-parameters: the trials of a tuning sweep as the environments of one batch
    def _proto_hyper(self):
        """the controller's own values as rows, in the expressions make_config uses for diagonal covariances"""
        from ..optim import is_plain

        ctrl, B, da = self.likelihood.controller, self.n_envs, self.likelihood.controller.dim_a
        a_cov = ctrl.a_dist.covariance_matrix
        lr = float(self._optim["lr"])
        rows = dict(lr=float(np.float32(lr)) if is_plain(self._optim) else lr,  # (dust_config carries a plain optimiser's lr in fp32)
                    alpha=np.float32(float(self.likelihood.alpha)), temperature=np.float32(float(ctrl.temp)),
                    sigma_a=a_cov.diag().sqrt().numpy().astype(np.float32), chol_a=torch.linalg.cholesky(a_cov).diag().numpy().astype(np.float32),
                    sigma_p=self._prior_cov.diag().sqrt().numpy().astype(np.float32), weighted_prior=int(bool(self.w_prior)))
        wide = ("sigma_a", "chol_a", "sigma_p")
        return {k: np.broadcast_to(np.asarray(v), (B, da) if k in wide else (B,)).copy() for k, v in rows.items()}

    def set_hyper(self, lr=None, alpha=None, temperature=None, prior_sigma=None, ctrl_sigma=None, weighted_prior=None):
        """Hyper-parameters per environment - the trials of the reference's demo/pendulum_tuning.py and demo/particle_tuning.py as the
        environments of ONE batch, so that a sweep is one run_episodes() call.  Each argument is None (the controller's own value), a
        scalar or [B]; the sigmas (standard deviations of the diagonal prior / action covariances) may be [B, dim_a].  alpha and
        temperature are independent: the scripts' temperature = 1 / alpha is the caller's line.  With every argument None the batch
        returns to the controller's values.  The horizon is not per environment (it shapes the launch): sweep it with one batch per
        value.  Raises ValueError before any device call for wrong lengths and for values that are not finite and > 0."""
        from ..optim import is_plain

        B, da = self.n_envs, self.likelihood.controller.dim_a
        given = dict(lr=lr, alpha=alpha, temperature=temperature, sigma_p=prior_sigma, sigma_a=ctrl_sigma, weighted_prior=weighted_prior)
        names = dict(sigma_p="prior_sigma", sigma_a="ctrl_sigma")
        if all(v is None for v in given.values()):
            self._hyper = None
            if self._batch is not None:
                self._batch.set_hyper(None)
            return
        rows = self._proto_hyper()
        for k, v in given.items():
            if v is None:
                continue
            name = names.get(k, k)
            v = np.asarray(torch.as_tensor(v).detach().numpy() if isinstance(v, torch.Tensor) else v)
            wide = k in ("sigma_a", "sigma_p")
            if v.ndim == 2 and wide and v.shape in ((B, 1), (B, da)):
                v = np.broadcast_to(v, (B, da))
            elif v.ndim == 1 and v.shape == (B,):
                v = np.broadcast_to(v[:, None], (B, da)) if wide else v
            elif v.ndim == 0:
                v = np.broadcast_to(v, (B, da) if wide else (B,))
            else:
                raise ValueError("%s has shape %s: a scalar or [%d]%s" % (name, v.shape, B, (" or [%d, %d]" % (B, da)) if wide else ""))
            if k == "weighted_prior":
                if not np.isin(v, (0, 1)).all():
                    raise ValueError("weighted_prior must be False / True (0 / 1)")
                rows[k] = v.astype(np.int64).copy()
                continue
            v = v.astype(np.float64)
            if not (np.isfinite(v).all() and (v > 0).all()):
                raise ValueError("%s must be finite and > 0" % name)
            if k == "lr":
                rows[k] = v.astype(np.float32).astype(np.float64) if is_plain(self._optim) else v.copy()
            else:
                rows[k] = v.astype(np.float32)  # fp32 sigma, as make_config forms it
            if not (rows[k] > 0).all() or not np.isfinite(rows[k]).all():
                raise ValueError("%s must be finite and > 0 in float32" % name)
            if k == "sigma_a":
                rows["chol_a"] = rows[k].copy()  # (diagonal: cholesky(a_cov) = sigma_a)
        self._hyper = rows
        if self._batch is not None:
            self._batch.set_hyper(rows)

    @property
    def hyper(self):
        """The rows in force as a dict of arrays: lr, alpha, temperature, weighted_prior [B]; sigma_a, chol_a, sigma_p [B, dim_a]"""
        if self._batch is not None:
            return self._batch.get_hyper()
        rows = self._proto_hyper() if self._hyper is None else self._hyper
        out = {k: np.array(v) for k, v in rows.items()}
        out["weighted_prior"] = np.asarray(out["weighted_prior"], np.int32)
        return out

    # -- the posterior's history: the reference's PolParticles / DynParticles rows (simulations.py:122, 134-137) out of the device episodes
    def set_history(self, theta=True, filter=False):
        """What simulate() records from now on (dust_svmpc_batch_set_history): `theta` - the particles after every period, written by the
        episode's own kernel (svmpc_sim_hist_kernel; no launch is added, nothing the episode computes changes); `filter` - the filters'
        particles, which only the dual loop has (BatchDualSVMPC.set_history).  Both False: recording off.  simulate()'s signature and
        result do not change: read the rows from `history`.  Deep copies carry the setting, not the rows."""
        self._history = (bool(theta), bool(filter))
        if self._batch is not None:
            self._batch.set_history(*self._history)

    @property
    def history(self):
        """{'theta': [T, B, N, H, da]} of the last recording simulate(): theta[t] is `theta` after period t (optimize() while the episode
        warms up, tick() afterwards); rows an environment did not run are NaN.  The library raises (DUST_ERR_STATE) while nothing is
        recorded."""
        from .. import _lib as L

        if self._batch is None:
            raise RuntimeError("nothing is recorded yet: set_history(), then simulate()")
        return {"theta": torch.from_numpy(self._batch.history(L.HIST_THETA))}

    def _history_refusals(self):
        """what a recording episode refuses, ahead of any device call: there is no recording instance for these two forms"""
        if not any(self._history):
            return
        from ..costs import cost_grid_key

        if self._hyper is not None:
            raise NotImplementedError("a recording episode has no per-environment hyper-parameters: set_history(False, False) first (or set_hyper())")
        if cost_grid_key(self.likelihood.controller.inst_cost_fn) is not None:
            raise NotImplementedError("a recording episode has no navigation cost: set_history(False, False) first")

    def __deepcopy__(self, memo):
        import copy

        new = copy.copy(self)
        memo[id(self)] = new
        for k, v in self.__dict__.items():
            if k == "_batch":
                new._batch = None if v is None else v.clone()
            elif k in ("kernel", "optimizer_class"):
                setattr(new, k, v)
            else:
                setattr(new, k, copy.deepcopy(v, memo))
        return new

    @property
    def theta(self):
        """[B, N, H, da]"""
        if self._batch is None:
            return self._theta0
        from .. import _lib as L

        return torch.from_numpy(self._batch.get(L.SVB_THETA))

    @theta.setter
    def theta(self, v):
        self._theta0 = torch.as_tensor(v, dtype=torch.float).detach().clone().reshape(self._theta0.shape)
        if self._batch is not None:
            from .. import _lib as L

            self._batch.set(L.SVB_THETA, self._theta0.numpy())

    def _states(self, states):
        return torch.as_tensor(states, dtype=torch.float).reshape(self.n_envs, -1).numpy()

    def _active(self, active):
        return _active(active, self.n_envs)

    def _params(self, params_dist, n_steps, on, params):
        """[B, n_steps, M, P]: the caller's rows, or the draws SVMPC makes, once per active environment in environment order"""
        ctrl = self.likelihood.controller
        if params is not None:
            return np.asarray(torch.as_tensor(params, dtype=torch.float).numpy(), np.float32)
        if not ctrl._sampling:
            return None
        rows = [ctrl._sample_params(params_dist, n_steps)[0] if on[b] else None for b in range(self.n_envs)]
        shape = next(r for r in rows if r is not None).shape if on.any() else (n_steps, ctrl.n_params, 1)
        return np.stack([np.zeros(shape, np.float32) if r is None else np.asarray(r, np.float32) for r in rows])

    def _eps(self, eps):
        return None if eps is None else np.asarray(eps, np.float32)

    # -- svmpc.py:87-126 for every environment
    def optimize(self, states, params_dist, n_steps=None, eps=None, active=None, params=None):
        """states [B, ds]; eps [B, n_steps, S, N, H, da] or None (device noise); params [B, n_steps, M, P] overrides the class's own
        draws from `params_dist` - one parameter distribution per environment."""
        check_optimizer(self.optimizer, self._opt_group)
        batch = self._ensure_batch(params_dist)
        n_steps = self.n_steps if n_steps is None else n_steps
        on = self._active(active)
        batch.optimize(self._states(states), n_steps, self._eps(eps), self._params(params_dist, n_steps, on, params), None if active is None else on)

    # -- svmpc.py:172-200 for every environment
    def forward(self, states, params_dist, active=None):
        """-> (a_seq [B, H, da], p_weights [B, N]); the rows of inactive environments are NaN"""
        batch = self._ensure_batch(params_dist)
        a_seq, pw = batch.forward(None if active is None else self._active(active))
        return torch.from_numpy(a_seq), torch.from_numpy(pw)

    def tick(self, states, params_dist, n_steps=None, eps=None, active=None, params=None):
        """optimize + forward of every active environment in ONE launch (dust_svmpc_batch_tick)"""
        check_optimizer(self.optimizer, self._opt_group)
        batch = self._ensure_batch(params_dist)
        n_steps = self.n_steps if n_steps is None else n_steps
        on = self._active(active)
        a_seq, pw = batch.tick(self._states(states), n_steps, self._eps(eps), self._params(params_dist, n_steps, on, params),
                               None if active is None else on)
        return torch.from_numpy(a_seq), torch.from_numpy(pw)

    # -- simulations.py:104-130 for every environment: optimize, forward, first action to the plant, new state, repeat
    def run_episodes(self, states, params_dist, n_periods, plant_params=None, n_steps=None, active=None, params=None):
        """`n_periods` closed-loop periods of every active environment in ONE launch (dust_svmpc_batch_episode): the plants are stepped
        on the device, with the first action of every period's sequence, by the model's own step under the environment's TRUE
        parameters `plant_params` [B, P] (the columns and the space of the controller's dynamics samples; None: the nominal model),
        without process noise.  states [B, ds]: where the episodes start.  The dynamics samples are drawn as `n_periods` successive
        draws of tick() in period order - under one torch.manual_seed the call consumes the torch stream exactly as `n_periods` calls
        of tick() do - unless `params` [T, B, n_steps, M, P] overrides them.
        -> (states [T, B, ds] after every step, actions [T, B, da], p_weights [T, B, N], a_seq [B, H, da] of the last period); the rows
        of inactive environments are NaN."""
        check_optimizer(self.optimizer, self._opt_group)
        ctrl = self.likelihood.controller
        T = int(n_periods)
        if not 1 <= T <= 4096:
            raise ValueError("n_periods = %d outside [1, 4096]: one launch runs one episode piece, split a longer one" % T)
        on = self._active(active)
        P = len(self.likelihood.model.uncertain_params or ()) if ctrl._sampling else 0
        if plant_params is not None:
            plant_params = np.asarray(torch.as_tensor(plant_params, dtype=torch.float).numpy(), np.float32)
            if P == 0 or plant_params.shape != (self.n_envs, P):
                raise ValueError("plant_params has shape %s, the plants read %s" % (plant_params.shape, (self.n_envs, P) if P else "none"))
        n_steps = self.n_steps if n_steps is None else n_steps
        batch = self._ensure_batch(params_dist)
        if params is not None:
            rows = np.asarray(torch.as_tensor(params, dtype=torch.float).numpy(), np.float32)
        elif ctrl._sampling:
            rows = np.stack([self._params(params_dist, n_steps, on, None) for _ in range(T)])
        else:
            rows = None
        xs, acts, pw, a_seq = batch.episode(self._states(states), T, n_steps, rows, plant_params, None if active is None else on)
        return torch.from_numpy(xs), torch.from_numpy(acts), torch.from_numpy(pw), torch.from_numpy(a_seq)

    # -- run_particle_episode / run_pendulum_simulation (simulations.py:104-130, 217-260) for every environment: the episode under the
    # reference's rules - warm-up, the accumulated cost, crash and goal
    def simulate(self, states, params_dist, n_periods, warm_up=0, goal=None, goal_radius=None, stop_on_crash=False, plant_params=None,
                 n_steps=None, active=None, params=None, resume=None):
        """run_episodes() under the reference's episode rules, still ONE launch (dust_svmpc_batch_simulate).  While the episode's period
        index is below `warm_up` a period is optimize() alone and the plant gets a zero action; the controller's instantaneous cost of
        every new state is recorded and summed in fp32 into `loss`, the quantity the tuning scripts minimise; `stop_on_crash`: a new
        position on an occupied cell of the model's (or the navigation cost's) map ends the environment with loss = inf, status 2;
        `goal` [ds] with `goal_radius` > 0: an environment within the radius ends with status 1.  `resume`: the result of a previous
        call - the episode goes on from its loss, status and period index (a changed plant, such as the reference's load at steps // 4,
        is two calls).  The dynamics samples are drawn as run_episodes() draws them: under one torch.manual_seed the call consumes the
        torch stream as `n_periods` calls of optimize() / tick() with the same `active` do.
        -> SimResult(states [T, B, ds], actions [T, B, da], p_weights [T, B, N], costs [T, B], loss [B], status [B], n_run [B], a_seq
        [B, H, da]) with the attribute t0 (the periods the episode has run); rows the call did not write - past n_run[b], warm-up rows
        of p_weights, inactive environments - are NaN (n_run: -1)."""
        check_optimizer(self.optimizer, self._opt_group)
        if self._history[0]:  # (with `filter` alone the plain episode records nothing)
            self._history_refusals()
        ctrl, model = self.likelihood.controller, self.likelihood.model
        T, warm_up = int(n_periods), int(warm_up)
        if not 1 <= T <= 4096:
            raise ValueError("n_periods = %d outside [1, 4096]: one launch runs one episode piece, split a longer one" % T)
        if warm_up < 0:
            raise ValueError("warm_up = %d < 0" % warm_up)
        on = self._active(active)
        P = len(model.uncertain_params or ()) if ctrl._sampling else 0
        if plant_params is not None:
            plant_params = np.asarray(torch.as_tensor(plant_params, dtype=torch.float).numpy(), np.float32)
            if P == 0 or plant_params.shape != (self.n_envs, P):
                raise ValueError("plant_params has shape %s, the plants read %s" % (plant_params.shape, (self.n_envs, P) if P else "none"))
        if (goal is None) != (goal_radius is None):
            raise ValueError("goal and goal_radius come together")
        if goal is not None:
            goal = np.asarray(torch.as_tensor(goal, dtype=torch.float).numpy(), np.float32).reshape(-1)
            if goal.shape != (ctrl.dim_s,) or not np.isfinite(goal).all():
                raise ValueError("goal has shape %s: [%d] finite entries" % (goal.shape, ctrl.dim_s))
            if not (np.isfinite(float(goal_radius)) and float(goal_radius) > 0):
                raise ValueError("goal_radius must be finite and > 0")
        if stop_on_crash:
            from ..costs import cost_grid_key

            has_map = (model.family == "particle" and bool(model.with_obstacle)) or cost_grid_key(ctrl.inst_cost_fn) is not None
            if not has_map:
                raise ValueError("stop_on_crash needs an occupancy map: Particle(with_obstacle=True) or a NavigationCost")
        t0, loss, status = 0, None, None
        if resume is not None:
            t0, loss, status = int(resume.t0), resume.loss.numpy(), resume.status.numpy()
            if loss.shape != (self.n_envs,) or status.shape != (self.n_envs,):
                raise ValueError("resume carries %d environments, the batch has %d" % (loss.size, self.n_envs))
        n_steps = self.n_steps if n_steps is None else n_steps
        batch = self._ensure_batch(params_dist)
        if params is not None:
            rows = np.asarray(torch.as_tensor(params, dtype=torch.float).numpy(), np.float32)
        elif ctrl._sampling:
            rows = np.stack([self._params(params_dist, n_steps, on, None) for _ in range(T)])
        else:
            rows = None
        out = batch.simulate(self._states(states), T, n_steps, rows, plant_params, t0=t0, warm_up=warm_up, goal=goal, goal_radius=goal_radius,
                             stop_on_crash=stop_on_crash, loss=loss, status=status, active=None if active is None else on)
        res = SimResult(*(torch.from_numpy(np.ascontiguousarray(v)) for v in out))
        res.t0 = t0 + T
        return res


class SimResult(collections.namedtuple("SimResult", "states actions p_weights costs loss status n_run a_seq")):
    """What BatchSVMPC.simulate returns; `t0`: the periods the episode has run so far (simulate(resume=) goes on from there)"""
    t0 = 0
