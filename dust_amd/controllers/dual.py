"""`DualSVMPC`: dual Stein-variational MPC as ONE object - the control-side SVGD (`SVMPC`) and the dynamics-side SVGD (`MPF`) composed
the way the reference composes them by hand in its simulation loop (dust/utils/simulations.py:104-138; demo/pendulum_example.py
"DuSt-MPC" case).  BASELINE.json's north_star names this surface ("DualSVMPC / SVMPC step() and forward()"); the reference has no
such class, so the names below are new and the SEMANTICS are the loop's:

    forward(state)            simulations.py:108-123   svmpc.optimize(state, dyn_dist); [step >= warm_up:] svmpc.forward(state, dyn_dist)
                                                        -> (a_seq [H, da], p_weights [N]); zero action sequence while warming up
    step(action, new_state)   simulations.py:132-138   mpf.optimize(action, new_state, bw, n_steps) -> (grad_norms, bw); the
                                                        controller's dynamics samples are drawn from the filter's refreshed prior
                                                        (dyn_dist = mpf.prior, simulations.py:79) from the next forward() on

Both halves run on the MI355X through the C ABI (dust_svmpc_tick / dust_svmpc_optimize + forward; dust_mpf_optimize;
dust_mpf_prior_sample).  `fused=True` (round 6) runs a whole control period - the filter update for the action just applied, Silverman's
bandwidth ON THE DEVICE when none is given, the controller's dynamics samples drawn from the refreshed filter prior on the device, the
control tick (a sigma-point controller, `MerweScaledUTF`: the sigma points of that prior, computed on the device; a custom `sqrt_method`
stays on the unfused path) - in ONE C call (dust_dual_tick): step() then only notes (action, new_state) and the next forward() carries it out; the
filter's particles are current again after that forward().  The draws come from the library's Philox stream (not torch's), so a run
with recorded draws (`draw_source`) stays on the unfused path.  `serve=True` turns on closed-loop serving for the control half when its shape allows it (nominal dynamics only:
a filter-coupled controller samples dynamics parameters per tick, which serving does not take - then it is a no-op)."""
import collections
import copy

import numpy as np
import torch


class DualSVMPC:
    def __init__(self, svmpc, mpf=None, dyn_dist=None, mpf_bw=None, mpf_steps=20, warm_up=0, n_steps=None, fused=False, seed=0):
        """svmpc: dust_amd.inference.SVMPC; mpf: dust_amd.inference.MPF or None (control half only: dyn_dist, possibly None, is then
        the fixed distribution the controller samples dynamics parameters from); mpf_bw: bandwidth handed to mpf.optimize (None:
        silvermans_rule of the filter's particles, mpf.py:68-73); n_steps: SVGD iterations per control tick (None: svmpc.n_steps)."""
        self.svmpc, self.mpf = svmpc, mpf
        self.dyn_dist = mpf.prior if mpf is not None else dyn_dist
        self.mpf_bw, self.mpf_steps = mpf_bw, int(mpf_steps)
        self.warm_up, self.n_steps = int(warm_up), n_steps
        self.ticks = 0
        self.last_bw = None
        self.fused, self._seed, self._pending = bool(fused), int(seed), None

    def __deepcopy__(self, memo):  # simulations.py:62,78: the loop deep-copies controller and filter per episode
        new = copy.copy(self)
        memo[id(self)] = new
        new.svmpc = copy.deepcopy(self.svmpc, memo)
        new.mpf = copy.deepcopy(self.mpf, memo)
        new.dyn_dist = new.mpf.prior if new.mpf is not None else self.dyn_dist
        return new

    # ---- attributes the loop reads (simulations.py:122, 140-160)
    @property
    def theta(self):
        return self.svmpc.theta

    @property
    def dyn_particles(self):
        if self.mpf is None:
            return None
        self._flush()
        return self.mpf.x

    @property
    def controller(self):
        return self.svmpc.likelihood.controller

    # ---- the control half of a tick (simulations.py:108-123)
    def _can_fuse(self):
        ctrl = self.controller
        tf = getattr(ctrl, "_tf", None)
        # a sigma-point controller: the device computes the points of the filter's diagonal prior for the default (Cholesky) root only
        if tf is not None and (self.mpf is None or not tf.default_sqrt or tf.n != self.mpf._dev.P):
            return False
        return (self.fused and self.mpf is not None and self.dyn_dist is self.mpf.prior and getattr(ctrl, "draw_source", None) is None
                and self.mpf.draw_source is None and self.svmpc.roll_strategy != "resample" and self.ticks >= self.warm_up)

    def forward(self, state):
        sv = self.svmpc
        if self._can_fuse():  # one C call: (pending filter update) -> dynamics samples on the device -> optimize + forward
            ctx = sv._ctx(self.dyn_dist)
            n_steps = sv.n_steps if self.n_steps is None else self.n_steps
            pend, self._pending = self._pending, None
            self._seed += 1
            a_prev = None if pend is None else pend[0]
            a_seq, pw, bw = ctx.dual_tick(self.mpf._dev, sv._state(state), a_prev, n_steps, self.mpf_steps, self.mpf_bw, self._seed)
            if pend is not None:
                self.last_bw = bw
            sv._prior_stale = True
            self.ticks += 1
            return torch.from_numpy(a_seq), torch.from_numpy(pw)
        self._flush()
        sv.optimize(state, self.dyn_dist, n_steps=self.n_steps)
        self.ticks += 1
        if self.ticks <= self.warm_up:  # the loop applies a zero action while the particles warm up and does NOT roll them
            return torch.zeros(self.controller.hz_len, self.controller.dim_a), None
        return sv.forward(state, self.dyn_dist)

    # ---- the dynamics half (simulations.py:132-138)
    def _flush(self):
        """A filter update noted by a fused step() and not carried out yet: run it now (the unfused path is about to read the filter)."""
        pend, self._pending = self._pending, None
        if pend is not None:
            a = torch.as_tensor(pend[0], dtype=torch.float).reshape(-1)
            _, self.last_bw = self.mpf.optimize(a.squeeze() if a.numel() == 1 else a, pend[1], bw=self.mpf_bw, n_steps=self.mpf_steps)

    def step(self, action, new_state):
        if self.mpf is None:
            return None, None
        if self._can_fuse():  # carried out by the next forward(new_state): one C call for the whole period
            self._flush()
            self._pending = (torch.as_tensor(action, dtype=torch.float).reshape(-1).numpy().copy(), torch.as_tensor(new_state, dtype=torch.float).reshape(-1).clone())
            return None, None
        a = torch.as_tensor(action, dtype=torch.float).reshape(-1)
        grads, bw = self.mpf.optimize(a.squeeze() if a.numel() == 1 else a, new_state, bw=self.mpf_bw, n_steps=self.mpf_steps)
        self.last_bw = bw
        return grads, bw

    def tick(self, state, plant):
        """One full loop iteration with a host plant callable `plant(state, action) -> new_state`: forward, plant, step.
        Returns (action, new_state, p_weights)."""
        a_seq, pw = self.forward(state)
        action = a_seq[0]
        new_state = plant(state, action)
        self.step(action, new_state)
        return action, new_state, pw


class DualAMPPI:
    """The dual loop over an `AMPPI` controller: the reference composes it by hand in its simulation loop (dust/utils/simulations.py:
    104-138 with dust/controllers/amppi.py:227-260 as the controller) -

        forward(state)            model.params_dist = mpf.prior; controller.update_actions(model, state)   -> (a_seq [H, da], omega [S]);
                                  controller.roll(roll) follows, so `a_seq` is the sequence BEFORE the roll (its row 0 is the action)
        step(action, new_state)   mpf.optimize(action, new_state, bw, n_steps)                              -> (grad_norms, bw)

    `fused=True` carries a whole period out in ONE C call (dust_amppi_dual_tick): step() only notes (action, new_state), the next
    forward() runs the filter update, Silverman's bandwidth on the device when none is given, the parameters from the refreshed prior
    ON THE DEVICE - "extended": every trajectory's row is drawn inside the tick's kernel, no S x P rows cross the bus; "single": one
    staged row; a `MerweScaledUTF`: the prior's sigma points -, the update and the roll.  Reading `dyn_particles` in between carries
    the noted update out first.  The fused draws come from the library's Philox stream under `seed` (one key per period).  A transform
    with a custom `sqrt_method`, or over another number of parameters than the filter's, stays on the unfused path.  Both paths draw the
    action noise on the device and return no rollouts (the controller's `return_rollouts` is not consulted: the loop reads `a_seq` and
    `omega` alone); `last_costs` holds the tick's costs.  Fused and unfused count their Philox keys alike (seed + 1, + 2, ... against the
    prior's own counter 1, 2, ...), so at `seed=0` and with a fixed `mpf_bw` the two run the same numbers."""

    def __init__(self, controller, model, mpf, mpf_bw=None, mpf_steps=20, fused=False, seed=0, roll=1):
        if getattr(controller, "_sample_shape", None) is None and getattr(controller, "_tf", None) is None:
            raise ValueError("DualAMPPI needs a controller that samples dynamics parameters: params_sampling='none' reads no filter")
        if bool(getattr(mpf.likelihood, "log_space", False)):
            raise NotImplementedError("a log-space filter under AMPPI: the controller hands samples to the model as drawn (amppi.py:134-139)")
        if int(roll) < 0:
            raise ValueError("roll=%d: roll >= 0" % roll)
        self.controller, self.model, self.mpf = controller, model, mpf
        self.mpf_bw, self.mpf_steps, self.roll = mpf_bw, int(mpf_steps), int(roll)
        self.fused, self._seed, self._pending = bool(fused), int(seed), None
        self.ticks = 0
        self.last_bw = None
        self.last_costs = None

    def __deepcopy__(self, memo):
        new = copy.copy(self)
        memo[id(self)] = new
        new.mpf = copy.deepcopy(self.mpf, memo)
        new.controller = copy.deepcopy(self.controller, memo)
        new.model = copy.deepcopy(self.model, memo)
        new.mpf.prior._seed = self.mpf.prior._seed  # (the unfused draws are keyed by the prior's own counter: the copy continues the stream)
        if getattr(self.model, "params_dist", None) is self.mpf.prior:
            new.model.params_dist = new.mpf.prior
        return new

    @property
    def a_seq(self):
        return self.controller.a_seq

    @property
    def dyn_particles(self):
        self._flush()
        return self.mpf.x

    def _can_fuse(self):
        tf = getattr(self.controller, "_tf", None)
        if tf is not None and (not tf.default_sqrt or tf.n != self.mpf._dev.P):
            return False
        return self.fused and self.mpf.draw_source is None

    def forward(self, state, actions=None):
        """actions [S, H, da]: recorded action samples in place of device-drawn noise (update_actions's third argument)"""
        ctrl = self.controller
        if self._can_fuse():
            self.model.params_dist = self.mpf.prior  # (what the context's configuration and an unfused period read)
            ctx = ctrl._ensure_ctx(self.model)
            if ctrl._tf is not None:
                ctx.set_sigma_scale(ctrl._tf.scale)
            pend = self._pending
            st = torch.as_tensor(state, dtype=torch.float).reshape(-1).numpy()
            acts = None if actions is None else torch.as_tensor(actions, dtype=torch.float).numpy()
            costs, omega, a_seq, _, bw = ctx.amppi_dual_tick(self.mpf._dev, st, None if pend is None else pend[0], acts,
                                                            shared_params=ctrl.params_sampling == "single", mpf_steps=self.mpf_steps,
                                                            mpf_bw=self.mpf_bw, seed=self._seed + 1, roll=self.roll)
            self._seed, self._pending = self._seed + 1, None  # (a refused call consumes neither the key nor the noted update)
            if pend is not None:
                self.last_bw = bw
            self.last_costs = torch.from_numpy(costs)
            self.ticks += 1
            return torch.from_numpy(a_seq), torch.from_numpy(omega)
        self._flush()
        self.model.params_dist = self.mpf.prior
        keep, ctrl.return_rollouts = ctrl.return_rollouts, False
        try:
            costs, _, _, omega = ctrl.update_actions(self.model, state, actions)
        finally:
            ctrl.return_rollouts = keep
        a_seq = ctrl.a_seq
        if self.roll > 0:
            ctrl.roll(self.roll)
        self.last_costs = costs
        self.ticks += 1
        return a_seq, omega

    def _flush(self):
        """A filter update noted by a fused step() and not carried out yet: run it now."""
        pend, self._pending = self._pending, None
        if pend is not None:
            a = torch.as_tensor(pend[0], dtype=torch.float).reshape(-1)
            _, self.last_bw = self.mpf.optimize(a.squeeze() if a.numel() == 1 else a, pend[1], bw=self.mpf_bw, n_steps=self.mpf_steps)

    def step(self, action, new_state):
        if self._can_fuse():  # carried out by the next forward(new_state)
            self._flush()
            self._pending = (torch.as_tensor(action, dtype=torch.float).reshape(-1).numpy().copy(),
                             torch.as_tensor(new_state, dtype=torch.float).reshape(-1).clone())
            return None, None
        a = torch.as_tensor(action, dtype=torch.float).reshape(-1)
        grads, bw = self.mpf.optimize(a.squeeze() if a.numel() == 1 else a, new_state, bw=self.mpf_bw, n_steps=self.mpf_steps)
        self.last_bw = bw
        return grads, bw

    def tick(self, state, plant):
        """One loop iteration with a host plant callable `plant(state, action) -> new_state`: forward, plant, step.
        Returns (action, new_state, omega)."""
        a_seq, omega = self.forward(state)
        action = a_seq[0]
        new_state = plant(state, action)
        self.step(action, new_state)
        return action, new_state, omega


class _BatchDual:
    """What the batched dual loops share: the B filters behind the prototype `mpf` (made by the first forward()), the prior keys of a
    period and the update a step() notes for the next forward().  A class copies its own parts in `_copy_parts(new, memo)`."""

    def __init__(self, n_envs, mpf, mpf_bw, mpf_steps, seed, init_particles):
        self.mpf, self.n_envs = mpf, n_envs
        self.mpf_bw, self.mpf_steps = mpf_bw, int(mpf_steps)
        self._seed, self._t, self._pending = int(seed), 0, None
        if init_particles is not None:
            init_particles = torch.as_tensor(init_particles, dtype=torch.float).detach().clone()
            want = (self.n_envs, mpf._dev.Mp, mpf._dev.P)
            if tuple(init_particles.shape) != want:
                raise ValueError("init_particles has shape %s, the batch takes %s" % (tuple(init_particles.shape), want))
        self._init_particles = init_particles
        self._mb = None
        self._filter_hyper = None
        self.ticks = 0
        self.last_bw = None

    def set_filter_hyper(self, rows):
        """Per-environment filter hyper-parameters (MpfBatch.set_hyper): a list of B dicts or a structured array [B] with any of lr,
        obs_std, bw, bw_scale, or None to clear.  Environment b's filter then updates under row b in every call of this object; the
        rows carry the bandwidths, so an object made with a positive `mpf_bw` refuses (before any device call)."""
        if rows is not None:
            if self.mpf_bw is not None and float(self.mpf_bw) > 0:
                raise ValueError("mpf_bw = %g was given to the constructor: with per-environment filter rows the rows carry the bandwidths - "
                                 "put it in the rows (bw) and construct with mpf_bw=None" % float(self.mpf_bw))
            if len(rows) != self.n_envs:
                raise ValueError("%d rows for %d environments" % (len(rows), self.n_envs))
            rows = rows.copy() if hasattr(rows, "dtype") else [dict(r) for r in rows]
        if self._mb is not None:
            self._mb.set_hyper(rows)
        self._filter_hyper = rows  # (the filters of an object that has not run yet take them when they are made)

    @property
    def filter_hyper(self):
        """The filter rows in force, a structured array [B] (MpfBatch.hyper): the prototype's values where none are set."""
        if self._mb is not None:
            return self._mb.hyper
        mb = self.mpf._dev.batch(self.n_envs)  # (the filters are made by the first forward(): ask a batch of their kind)
        try:
            if self._filter_hyper is not None:
                mb.set_hyper(self._filter_hyper)
            return mb.hyper
        finally:
            mb.close()

    def prior_keys(self, t):
        """The Philox keys of period t = 1, 2, ...: seed + (b << 32) + t for environment b (modulo 2^64)."""
        return [(self._seed + (b << 32) + int(t)) & 0xFFFFFFFFFFFFFFFF for b in range(self.n_envs)]

    def __deepcopy__(self, memo):
        new = copy.copy(self)
        memo[id(self)] = new
        self._copy_parts(new, memo)
        new._mb = None if self._mb is None else self._mb.clone()
        new._pending = None if self._pending is None else tuple(v.copy() for v in self._pending)
        return new

    def _filters(self, states=None):
        if self._mb is None:
            if self.mpf.draw_source is not None:
                raise NotImplementedError("recorded filter draws (draw_source) have no batched form")
            mb = self.mpf._dev.batch(self.n_envs)
            if self._init_particles is not None:
                mb.set_particles(self._init_particles.numpy())
            if states is not None:
                mb.set_obs(states)
            if self._filter_hyper is not None:
                mb.set_hyper(self._filter_hyper)
            self._mb = mb
        return self._mb

    @property
    def dyn_particles(self):
        """[B, Mp, P]; a noted update is carried out first"""
        self._flush()
        return torch.from_numpy(self._filters().get_particles())

    def _flush(self):
        pend = self._pending
        if pend is not None:
            _, bw = self._filters().optimize(pend[0], pend[1], self.mpf_bw, self.mpf_steps)
            self._pending, self.last_bw = None, torch.from_numpy(bw)

    def step(self, actions, new_states):
        self._flush()
        B = self.n_envs
        self._pending = (torch.as_tensor(actions, dtype=torch.float).reshape(B, -1).numpy().copy(),
                         torch.as_tensor(new_states, dtype=torch.float).reshape(B, -1).numpy().copy())
        return None, None


class BatchDualAMPPI(_BatchDual):
    """The dual loop over `B = controller.n_envs` plants at once: a `BatchAMPPI` and B copies of one `MPF` - the deep copies of controller
    and filter the reference makes per episode (dust/utils/simulations.py:62,78) - with a whole control period of all of them in ONE C
    call (dust_amppi_dual_batch_tick): the B filter updates in one launch, Silverman's bandwidths on the device when none is given, the
    parameters from every refreshed prior on the device, the B ticks in one launch, the roll.  Environment b runs what a
    `DualAMPPI(fused=True)` over `AMPPI(seed=seeds[b])` and a filter of its own runs, bit for bit when that filter takes the
    single-workgroup kernel (DUST_MPF_GRID=0), under the prior keys `seed + (b << 32) + t` in period t = 1, 2, ...: the lone class's
    `seed + t` on a per-environment base, so that two environments never meet on one key at different times.

        forward(states, actions=None, active=None)   -> (a_seq [B, H, da] before the roll, omega [B, S]); NaN rows for inactive environments
        step(actions [B, da], new_states [B, ds])    notes the update; the next forward() carries it out
        tick(states, plant)                          forward, `plant(states, actions) -> new_states`, step

    `mpf` is the prototype: every environment starts from its particles (or from `init_particles[b]`, [B, Mp, P]), optimiser state and
    bandwidths; the first forward()'s states are the observations the first update's predictions start from.  There is no unfused path:
    what the fused call does not take is refused."""

    def __init__(self, controller, model, mpf, mpf_bw=None, mpf_steps=20, seed=0, roll=1, init_particles=None):
        from .amppi import BatchAMPPI

        if not isinstance(controller, BatchAMPPI):
            raise TypeError("BatchDualAMPPI needs a BatchAMPPI controller, got %s" % type(controller).__name__)
        if getattr(controller, "_sample_shape", None) is None and getattr(controller, "_tf", None) is None:
            raise ValueError("BatchDualAMPPI needs a controller that samples dynamics parameters: params_sampling='none' reads no filter")
        if bool(getattr(mpf.likelihood, "log_space", False)):
            raise NotImplementedError("a log-space filter under AMPPI: the controller hands samples to the model as drawn (amppi.py:134-139)")
        if int(roll) < 0:
            raise ValueError("roll=%d: roll >= 0" % roll)
        tf = getattr(controller, "_tf", None)
        if tf is not None and (not tf.default_sqrt or tf.n != mpf._dev.P):
            raise NotImplementedError("a sigma-point transform with a custom sqrt_method, or over another number of parameters than the "
                                      "filter's, has no fused form - and a batch has no other")
        _BatchDual.__init__(self, controller.n_envs, mpf, mpf_bw, mpf_steps, seed, init_particles)
        self.controller, self.model, self.roll = controller, model, int(roll)
        self.last_costs = None

    def _copy_parts(self, new, memo):
        new.controller = copy.deepcopy(self.controller, memo)
        new.model = copy.deepcopy(self.model, memo)
        new.mpf = copy.deepcopy(self.mpf, memo)
        if getattr(self.model, "params_dist", None) is self.mpf.prior:
            new.model.params_dist = new.mpf.prior

    @property
    def a_seq(self):
        """[B, H, da]"""
        return self.controller.a_seq

    def forward(self, states, actions=None, active=None):
        """actions [B, S, H, da]: recorded action samples in place of device-drawn noise; active [B]: the environments that tick"""
        ctrl = self.controller
        self.model.params_dist = self.mpf.prior  # (what the context's configuration reads)
        batch = ctrl._ensure_batch(self.model)
        if ctrl._tf is not None:
            batch.ctx.set_sigma_scale(ctrl._tf.scale)
        st = torch.as_tensor(states, dtype=torch.float).reshape(self.n_envs, -1).numpy()
        mb = self._filters(st)
        acts = None if actions is None else torch.as_tensor(actions, dtype=torch.float).numpy()
        pend = self._pending
        costs, omega, a_seq, _, bw = batch.dual_tick(mb, st, None if pend is None else pend[0], acts,
                                                     shared_params=ctrl.params_sampling == "single", mpf_steps=self.mpf_steps,
                                                     mpf_bw=self.mpf_bw, seeds=self.prior_keys(self._t + 1), roll=self.roll, active=active)
        self._t, self._pending = self._t + 1, None  # (a refused call consumes neither the keys nor the noted update)
        if pend is not None:
            self.last_bw = torch.from_numpy(bw)
        self.last_costs = torch.from_numpy(costs)
        self.ticks += 1
        return torch.from_numpy(a_seq), torch.from_numpy(omega)

    def tick(self, states, plant):
        """One loop iteration with a host plant callable `plant(states [B, ds], actions [B, da]) -> new_states [B, ds]`: forward,
        plant, step.  Returns (actions, new_states, omega)."""
        a_seq, omega = self.forward(states)
        actions = a_seq[:, 0]
        new_states = plant(states, actions)
        self.step(actions, new_states)
        return actions, new_states, omega

    # -- simulations.py:104-138 for every environment, the plants on the device
    def run_episodes(self, states, n_periods, plant_params=None, active=None):
        """`n_periods` control periods of every active environment in one C call (dust_amppi_dual_batch_episode): what `n_periods` calls
        of tick() run, with the plants stepped on the device by the model's own step under the environment's TRUE parameters
        `plant_params` [B, P] (the columns of the filters' particles; None: the nominal model), without process or observation noise -
        no host round trip between the periods.  states [B, ds]: where the piece starts; a noted update is period 0's, with `states`
        as its observation, as in forward().  Period t draws under `prior_keys(_t + 1 + t)`, the key schedule of
        `BatchDualSVMPC.run_episodes`.  The roll is the constructor's `roll`, which must be >= 1 here.
        -> (states [T, B, ds] after every step, actions [T, B, da], costs [T, B, S], omega [T, B, S]); the rows of inactive
        environments are NaN.  Afterwards (actions[-1], states[-1]) is the noted update: forward(states[-1]), tick() or another
        run_episodes(states[-1], ...) continue the same loop.  Pendulum and Particle; a skid-steer or cart-pole pair is refused
        (tick() runs those)."""
        from ..models import CartPoleModel, SkidSteerRobot
        from ..inference.svmpc import _active

        ctrl = self.controller
        T = int(n_periods)
        if not 1 <= T <= 4096:
            raise ValueError("n_periods = %d outside [1, 4096]: one call runs one episode piece, chain a longer one" % T)
        if self.roll < 1:
            raise ValueError("run_episodes rolls every period: roll=%d, roll >= 1" % self.roll)
        for model in (self.model, getattr(self.mpf.likelihood, "model", None)):
            if isinstance(model, (SkidSteerRobot, CartPoleModel)):
                raise NotImplementedError("run_episodes conditions the filters on the device: Pendulum and Particle (a %s pair runs tick())"
                                          % type(model).__name__)
        on = None if active is None else _active(active, self.n_envs)
        P = self.mpf._dev.P
        if plant_params is not None:
            plant_params = np.asarray(torch.as_tensor(plant_params, dtype=torch.float).numpy(), np.float32)
            if plant_params.shape != (self.n_envs, P):
                raise ValueError("plant_params has shape %s, the plants read %s" % (plant_params.shape, (self.n_envs, P)))
        self.model.params_dist = self.mpf.prior  # (what the context's configuration reads)
        batch = ctrl._ensure_batch(self.model)
        if ctrl._tf is not None:
            batch.ctx.set_sigma_scale(ctrl._tf.scale)
        st = torch.as_tensor(states, dtype=torch.float).reshape(self.n_envs, -1).numpy()
        mb = self._filters(st)
        pend = self._pending
        keys = np.array([self.prior_keys(self._t + 1 + t) for t in range(T)], np.uint64)
        xs, acts, costs, omega, bw, _ = batch.dual_episode(mb, st, T, None if pend is None else pend[0],
                                                           shared_params=ctrl.params_sampling == "single", mpf_steps=self.mpf_steps,
                                                           mpf_bw=self.mpf_bw, seeds=keys, roll_steps=self.roll, plant_params=plant_params, active=on)
        # (a refused call consumes neither the keys nor the noted update)
        a_last, x_last = acts[-1].copy(), xs[-1].copy()
        if on is not None:  # an inactive environment keeps the pair it came with
            off = ~on
            a_last[off], x_last[off] = (0.0 if pend is None else pend[0][off]), st[off]
        self._t, self._pending = self._t + T, (a_last, x_last)
        if pend is not None or T > 1:
            self.last_bw = torch.from_numpy(bw[-1].copy())
        self.last_costs = torch.from_numpy(costs[-1].copy())
        self.ticks += T
        return torch.from_numpy(xs), torch.from_numpy(acts), torch.from_numpy(costs), torch.from_numpy(omega)

    # -- run_pendulum_simulation(mpf=...)'s AMPPI loop / the Particle loop's crash and goal (simulations.py:124-160, 217-260) for every
    # environment: the episode under the reference's rules; this branch has no warm-up
    def simulate(self, states, n_periods, goal=None, goal_radius=None, stop_on_crash=False, plant_params=None, active=None, resume=None):
        """run_episodes() under the reference's episode rules, in one C call (dust_amppi_dual_batch_simulate): the controller's
        instantaneous cost of every new state is recorded and summed in fp32 into `loss`; `stop_on_crash` (Particle with_obstacle): a new
        position on an occupied cell ends the environment with loss = inf, status 2; `goal` [ds] with `goal_radius` > 0: an environment
        within the radius ends with status 1.  A stopped environment takes no further filter update and no tick; environments with
        `resume.status != 0` are passed as inactive.  Period t draws under `prior_keys(_t + 1 + t)`; the roll is the constructor's
        `roll`, which must be >= 1 here.
        -> DualAmppiSimResult(states [T, B, ds], actions [T, B, da], costs [T, B, S], omega [T, B, S], bw [T, B], inst_costs [T, B], loss
        [B], status [B], n_run [B], a_seq [B, H, da]) with the attribute t0; rows the call did not write - past n_run[b], inactive
        environments - are NaN (n_run: -1).  Afterwards the noted update is, per environment, (actions[n_run - 1], states[n_run - 1]),
        or the pair the environment came with when n_run <= 0."""
        from ..inference.svmpc import _active
        from ..models import CartPoleModel, SkidSteerRobot
        from .amppi import DualAmppiSimResult, _sim_goal, _sim_resume

        ctrl = self.controller
        T, B = int(n_periods), self.n_envs
        if not 1 <= T <= 4096:
            raise ValueError("n_periods = %d outside [1, 4096]: one call runs one episode piece, chain a longer one" % T)
        if self.roll < 1:
            raise ValueError("simulate rolls every period: roll=%d, roll >= 1" % self.roll)
        for model in (self.model, getattr(self.mpf.likelihood, "model", None)):
            if isinstance(model, (SkidSteerRobot, CartPoleModel)):
                raise NotImplementedError("simulate conditions the filters on the device: Pendulum and Particle (a %s pair runs tick())"
                                          % type(model).__name__)
        on = np.ones(B, bool) if active is None else np.array(_active(active, B), bool)
        P = self.mpf._dev.P
        if plant_params is not None:
            plant_params = np.asarray(torch.as_tensor(plant_params, dtype=torch.float).numpy(), np.float32)
            if plant_params.shape != (B, P):
                raise ValueError("plant_params has shape %s, the plants read %s" % (plant_params.shape, (B, P)))
        goal, goal_radius = _sim_goal(goal, goal_radius, ctrl.dim_s)
        if stop_on_crash and not (getattr(self.model, "family", None) == "particle" and bool(self.model.with_obstacle)):
            raise ValueError("stop_on_crash needs an occupancy map: Particle(with_obstacle=True)")
        t0, loss, status = _sim_resume(resume, B)
        if status is not None:
            on = on & (status == 0)
        self.model.params_dist = self.mpf.prior  # (what the context's configuration reads)
        batch = ctrl._ensure_batch(self.model)
        if ctrl._tf is not None:
            batch.ctx.set_sigma_scale(ctrl._tf.scale)
        st = torch.as_tensor(states, dtype=torch.float).reshape(B, -1).numpy()
        mb = self._filters(st)
        pend = self._pending
        keys = np.array([self.prior_keys(self._t + 1 + t) for t in range(T)], np.uint64)
        masked = active is not None or resume is not None
        out = batch.dual_simulate(mb, st, T, None if pend is None else pend[0], shared_params=ctrl.params_sampling == "single",
                                  mpf_steps=self.mpf_steps, mpf_bw=self.mpf_bw, seeds=keys, roll_steps=self.roll, plant_params=plant_params,
                                  t0=t0, goal=goal, goal_radius=goal_radius, stop_on_crash=stop_on_crash, loss=loss, status=status,
                                  active=on if masked else None)
        # (a refused call consumes neither the keys nor the noted update)
        xs, acts, costs, omega, bw, ic, loss, status, n_run, a_seq = out
        a_last = np.zeros((B, acts.shape[2]), np.float32) if pend is None else pend[0].copy()
        x_last = np.array(st, np.float32).reshape(B, -1).copy()
        for e in range(B):
            n = int(n_run[e])
            if n > 0:  # (n <= 0: the environment keeps the pair it came with)
                a_last[e], x_last[e] = acts[n - 1, e], xs[n - 1, e]
        have = pend is not None or bool((n_run > 0).any())
        self._t, self._pending = self._t + T, ((a_last, x_last) if have else None)
        full = n_run == T
        if (pend is not None or T > 1) and bool(full.any()):
            self.last_bw = torch.from_numpy(bw[-1].copy())
        if bool(full.any()):
            self.last_costs = torch.from_numpy(costs[-1].copy())
        self.ticks += T
        res = DualAmppiSimResult(*(torch.from_numpy(np.ascontiguousarray(v)) for v in (xs, acts, costs, omega, bw, ic, loss, status, n_run, a_seq)))
        res.t0 = t0 + T
        return res


class BatchDualSVMPC(_BatchDual):
    """The DuSt-MPC loop over `B = svmpc.n_envs` plants at once: a `BatchSVMPC` and B copies of one `MPF` - the deep copies of controller
    and filter the reference makes per episode (dust/utils/simulations.py:62,78) - with a whole control period of all of them in ONE C
    call (dust_svmpc_dual_batch_tick): the B filter updates in one launch, Silverman's bandwidths on the device when none is given, then
    the B ticks (n_steps SVGD iterations and forward()) in one launch whose workgroups draw their dynamics samples from their own
    environment's refreshed prior.  Nothing crosses the bus between the filters and the ticks, and the launch count does not depend on B.
    Environment b draws what a `DualSVMPC(fused=True, seed=seed + (b << 32))` over a filter of its own draws, bit for bit when that
    filter takes the single-workgroup kernel, under the prior keys `seed + (b << 32) + t` in period t = 1, 2, ...: the lone class's
    `seed + t` on a per-environment base, so that two environments never meet on one key at different times.  (The lone and the batched
    SVMPC kernels add in different orders: the controllers agree to rounding.)

        forward(states, eps=None, active=None)      -> (a_seq [B, H, da]: the best particle before the roll, p_weights [B, N]); NaN rows
                                                    for inactive environments
        step(actions [B, da], new_states [B, ds])   notes the update; the next forward() carries it out
        tick(states, plant)                         forward, `plant(states, actions) -> new_states`, step

    `mpf` is the prototype: every environment starts from its particles (or from `init_particles[b]`, [B, Mp, P]), optimiser state and
    bandwidths; the first forward()'s states are the observations the first update's predictions start from.
    There is no unfused path: what the fused call does not take (a sigma-point controller, recorded draws) is refused.  `warm_up`
    (simulations.py:104-117):
    while `ticks < warm_up` forward() is a warm-up period (dust_svmpc_dual_batch_optimize) - the filters update, the particles take
    their SVGD iterations, nothing rolls - and returns a zero a_seq and None for the weights, the lone `DualSVMPC.forward` contract.
    The controller's cost is any `BatchSVMPC` runs: a skid-steer `NavigationCost` ticks in svmpc_skid_nav_prior_batch_kernel, one map
    for the B robots.  simulate() is the whole episode under the reference's rules in one C call."""

    def __init__(self, svmpc, mpf, mpf_bw=None, mpf_steps=20, n_steps=None, seed=0, init_particles=None, warm_up=0):
        from ..inference.svmpc import BatchSVMPC

        if not isinstance(svmpc, BatchSVMPC):
            raise TypeError("BatchDualSVMPC needs a BatchSVMPC controller, got %s" % type(svmpc).__name__)
        if not svmpc.likelihood.controller._sampling:
            raise ValueError("BatchDualSVMPC needs a controller that samples dynamics parameters: params_sampling=None reads no filter")
        if mpf.draw_source is not None:
            raise NotImplementedError("recorded filter draws (draw_source) have no batched form")
        self._no_rows(svmpc)
        if int(warm_up) < 0:
            raise ValueError("warm_up = %d < 0" % int(warm_up))
        _BatchDual.__init__(self, svmpc.n_envs, mpf, mpf_bw, mpf_steps, seed, init_particles)
        self.svmpc, self.n_steps, self.warm_up = svmpc, n_steps, int(warm_up)

    @staticmethod
    def _no_rows(svmpc):
        """the dual loop's kernels read launch-uniform hyper-parameters: refused ahead of any device call"""
        if getattr(svmpc, "_hyper", None) is not None:
            raise NotImplementedError("the dual loop has no per-environment hyper-parameters: BatchSVMPC.set_hyper() with no argument first")

    def _copy_parts(self, new, memo):
        new.svmpc = copy.deepcopy(self.svmpc, memo)
        new.mpf = copy.deepcopy(self.mpf, memo)

    @property
    def theta(self):
        """[B, N, H, da]"""
        return self.svmpc.theta

    @property
    def controller(self):
        return self.svmpc.likelihood.controller

    # -- the posterior's history: the reference's PolParticles / DynParticles rows (simulations.py:122, 134-137) out of simulate()
    def set_history(self, theta=True, filter=True):
        """What simulate() records from now on (BatchSVMPC.set_history, dust_svmpc_batch_set_history): `theta` - the controllers'
        particles after every period; `filter` - the filters' particles every period's tick drew its dynamics samples from.  Written by
        the period's own kernel (svmpc_dual_sim_hist_period_kernel): no launch is added and nothing the episode computes changes.  Both
        False: recording off.  simulate()'s signature and result do not change: read the rows from `history`.  Deep copies carry the
        setting, not the rows."""
        self.svmpc.set_history(theta, filter)

    @property
    def history(self):
        """The rows of the last recording simulate(), the kinds that were asked for: 'theta' [T, B, N, H, da] - `theta` after period t -
        and 'dyn_particles' [T, B, Mp, P] - the filters' particles after period t's update, before the pair (actions[t], states[t]) is
        folded in (in a period 0 without a noted update: the particles at entry).  Rows an environment did not run are NaN."""
        from .. import _lib as L

        sv = self.svmpc
        if sv._batch is None:
            raise RuntimeError("nothing is recorded yet: set_history(), then simulate()")
        out = {}
        if sv._history[0]:
            out["theta"] = torch.from_numpy(sv._batch.history(L.HIST_THETA))
        if sv._history[1]:
            out["dyn_particles"] = torch.from_numpy(sv._batch.history(L.HIST_FILTER))
        return out

    def forward(self, states, eps=None, active=None):
        """eps [B, n_steps, S, N, H, da]: recorded noise in place of device-drawn noise; active [B]: the environments that tick"""
        from ..inference.svmpc import check_optimizer

        sv = self.svmpc
        self._no_rows(sv)
        check_optimizer(sv.optimizer, sv._opt_group)
        batch = sv._ensure_batch(self.mpf.prior)
        n_steps = sv.n_steps if self.n_steps is None else self.n_steps
        st = sv._states(states)
        mb = self._filters(st)
        pend = self._pending
        if self.ticks < self.warm_up:  # a warm-up period: no forward(), a zero sequence for the plant (DualSVMPC.forward's contract)
            _, bw = batch.dual_optimize(mb, st, None if pend is None else pend[0], n_steps=n_steps, eps=sv._eps(eps),
                                        mpf_steps=self.mpf_steps, mpf_bw=self.mpf_bw, seeds=self.prior_keys(self._t + 1),
                                        active=None if active is None else sv._active(active))
            a_seq, pw = np.zeros((self.n_envs, batch.H, batch.da), np.float32), None
        else:
            a_seq, pw, _, bw = batch.dual_tick(mb, st, None if pend is None else pend[0], n_steps=n_steps, eps=sv._eps(eps),
                                               mpf_steps=self.mpf_steps, mpf_bw=self.mpf_bw, seeds=self.prior_keys(self._t + 1),
                                               active=None if active is None else sv._active(active))
        self._t, self._pending = self._t + 1, None  # (a refused call consumes neither the keys nor the noted update)
        if pend is not None:
            self.last_bw = torch.from_numpy(bw)
        self.ticks += 1
        return torch.from_numpy(a_seq), None if pw is None else torch.from_numpy(pw)

    def tick(self, states, plant):
        """One loop iteration with a host plant callable `plant(states [B, ds], actions [B, da]) -> new_states [B, ds]`: forward,
        plant, step.  Returns (actions, new_states, p_weights)."""
        a_seq, pw = self.forward(states)
        actions = a_seq[:, 0]
        new_states = plant(states, actions)
        self.step(actions, new_states)
        return actions, new_states, pw

    # -- simulations.py:104-138 for every environment, the plants on the device
    def run_episodes(self, states, n_periods, plant_params=None, n_steps=None, active=None):
        """`n_periods` control periods of every active environment in one C call (dust_svmpc_dual_batch_episode): what `n_periods` calls
        of tick() run, with the plants stepped on the device by the model's own step under the environment's TRUE parameters
        `plant_params` [B, P] (the columns and the space of the filters' particles; None: the nominal model), without process or
        observation noise - no host round trip between the periods.  states [B, ds]: where the piece starts; a noted update is period
        0's, with `states` as its observation, as in forward().  Period t draws under `prior_keys(_t + 1 + t)`.
        -> (states [T, B, ds] after every step, actions [T, B, da], p_weights [T, B, N], a_seq [B, H, da] of the last period); the rows
        of inactive environments are NaN.  Afterwards (actions[-1], states[-1]) is the noted update: forward(states[-1]), tick() or
        another run_episodes(states[-1], ...) continue the same loop.  Pendulum and Particle; a skid-steer or cart-pole pair is refused
        (tick() runs those)."""
        from ..inference.svmpc import check_optimizer
        from ..models import CartPoleModel, SkidSteerRobot

        sv = self.svmpc
        self._no_rows(sv)
        T = int(n_periods)
        if not 1 <= T <= 4096:
            raise ValueError("n_periods = %d outside [1, 4096]: one call runs one episode piece, chain a longer one" % T)
        for model in (sv.likelihood.model, getattr(self.mpf.likelihood, "model", None)):
            if isinstance(model, (SkidSteerRobot, CartPoleModel)):
                raise NotImplementedError("run_episodes conditions the filters on the device: Pendulum and Particle (a %s pair runs tick())"
                                          % type(model).__name__)
        P = self.mpf._dev.P
        if plant_params is not None:
            plant_params = np.asarray(torch.as_tensor(plant_params, dtype=torch.float).numpy(), np.float32)
            if plant_params.shape != (self.n_envs, P):
                raise ValueError("plant_params has shape %s, the plants read %s" % (plant_params.shape, (self.n_envs, P)))
        check_optimizer(sv.optimizer, sv._opt_group)
        batch = sv._ensure_batch(self.mpf.prior)
        if n_steps is None:
            n_steps = sv.n_steps if self.n_steps is None else self.n_steps
        st = sv._states(states)
        mb = self._filters(st)
        pend = self._pending
        keys = np.array([self.prior_keys(self._t + 1 + t) for t in range(T)], np.uint64)
        xs, acts, pw, bw, a_seq = batch.dual_episode(mb, st, T, n_steps, None if pend is None else pend[0], mpf_steps=self.mpf_steps,
                                                     mpf_bw=self.mpf_bw, seeds=keys, plant_params=plant_params,
                                                     active=None if active is None else sv._active(active))
        # (a refused call consumes neither the keys nor the noted update)
        a_last, x_last = acts[-1].copy(), xs[-1].copy()
        if active is not None:  # an inactive environment keeps the pair it came with
            off = ~sv._active(active)
            a_last[off], x_last[off] = (0.0 if pend is None else pend[0][off]), st[off]
        self._t, self._pending = self._t + T, (a_last, x_last)
        if pend is not None or T > 1:
            self.last_bw = torch.from_numpy(bw[-1].copy())
        self.ticks += T
        return torch.from_numpy(xs), torch.from_numpy(acts), torch.from_numpy(pw), torch.from_numpy(a_seq)

    # -- run_pendulum_simulation(mpf=...) / the Particle loop of demo/particle_example.py for every environment: the episode under the
    # reference's rules - warm-up with the filters updating, the accumulated cost, crash and goal
    def simulate(self, states, n_periods, goal=None, goal_radius=None, stop_on_crash=False, plant_params=None, n_steps=None, active=None,
                 resume=None):
        """run_episodes() under the reference's episode rules, in one C call (dust_svmpc_dual_batch_simulate).  The period index starts at
        `resume.t0` (0 without `resume`); while it is below `self.warm_up` a period is forward()'s warm-up period - the filters update,
        the plant gets a zero action; the controller's instantaneous cost of every new state is recorded and summed in fp32 into `loss`;
        `stop_on_crash` (Particle with_obstacle): a new position on an occupied cell ends the environment with loss = inf, status 2;
        `goal` [ds] with `goal_radius` > 0: an environment within the radius ends with status 1.  A stopped environment takes no
        further filter update and no tick; environments with `resume.status != 0` are passed as inactive.  Period t draws under
        `prior_keys(_t + 1 + t)`.
        -> DualSimResult(states [T, B, ds], actions [T, B, da], p_weights [T, B, N], bw [T, B], costs [T, B], loss [B], status [B],
        n_run [B], a_seq [B, H, da]) with the attribute t0; rows the call did not write - past n_run[b], warm-up rows of p_weights,
        inactive environments - are NaN (n_run: -1).  Afterwards the noted update is, per environment, (actions[n_run - 1],
        states[n_run - 1]), or the pair the environment came with when n_run <= 0.  The filters' particles are recorded per period
        only after set_history() (read `history`); `dyn_particles` reads them after the call (and carries the noted update out first)."""
        from ..inference.svmpc import check_optimizer
        from ..models import CartPoleModel, SkidSteerRobot

        sv = self.svmpc
        self._no_rows(sv)
        sv._history_refusals()
        ctrl, model = sv.likelihood.controller, sv.likelihood.model
        T = int(n_periods)
        if not 1 <= T <= 4096:
            raise ValueError("n_periods = %d outside [1, 4096]: one call runs one episode piece, chain a longer one" % T)
        for mdl in (model, getattr(self.mpf.likelihood, "model", None)):
            if isinstance(mdl, (SkidSteerRobot, CartPoleModel)):
                raise NotImplementedError("simulate conditions the filters on the device: Pendulum and Particle (a %s pair runs tick())"
                                          % type(mdl).__name__)
        P = self.mpf._dev.P
        if plant_params is not None:
            plant_params = np.asarray(torch.as_tensor(plant_params, dtype=torch.float).numpy(), np.float32)
            if plant_params.shape != (self.n_envs, P):
                raise ValueError("plant_params has shape %s, the plants read %s" % (plant_params.shape, (self.n_envs, P)))
        if (goal is None) != (goal_radius is None):
            raise ValueError("goal and goal_radius come together")
        if goal is not None:
            goal = np.asarray(torch.as_tensor(goal, dtype=torch.float).numpy(), np.float32).reshape(-1)
            if goal.shape != (ctrl.dim_s,) or not np.isfinite(goal).all():
                raise ValueError("goal has shape %s: [%d] finite entries" % (goal.shape, ctrl.dim_s))
            if not (np.isfinite(float(goal_radius)) and float(goal_radius) > 0):
                raise ValueError("goal_radius must be finite and > 0")
        if stop_on_crash and not (model.family == "particle" and bool(model.with_obstacle)):
            raise ValueError("stop_on_crash needs an occupancy map: Particle(with_obstacle=True)")
        B = self.n_envs
        on = np.ones(B, bool) if active is None else np.array(sv._active(active), bool)
        t0, loss, status = 0, None, None
        if resume is not None:
            t0, loss, status = int(resume.t0), resume.loss.numpy(), resume.status.numpy()
            if loss.shape != (B,) or status.shape != (B,):
                raise ValueError("resume carries %d environments, the batch has %d" % (loss.size, B))
            on = on & (status == 0)
        check_optimizer(sv.optimizer, sv._opt_group)
        batch = sv._ensure_batch(self.mpf.prior)
        if n_steps is None:
            n_steps = sv.n_steps if self.n_steps is None else self.n_steps
        st = sv._states(states)
        mb = self._filters(st)
        pend = self._pending
        keys = np.array([self.prior_keys(self._t + 1 + t) for t in range(T)], np.uint64)
        masked = active is not None or resume is not None
        out = batch.dual_simulate(mb, st, T, n_steps, None if pend is None else pend[0], mpf_steps=self.mpf_steps, mpf_bw=self.mpf_bw,
                                  seeds=keys, plant_params=plant_params, t0=t0, warm_up=self.warm_up, goal=goal, goal_radius=goal_radius,
                                  stop_on_crash=stop_on_crash, loss=loss, status=status, active=on if masked else None)
        # (a refused call consumes neither the keys nor the noted update)
        xs, acts, pw, bw, costs, loss, status, n_run, a_seq = out
        a_last = np.zeros((B, acts.shape[2]), np.float32) if pend is None else pend[0].copy()
        x_last = np.array(st, np.float32).reshape(B, -1).copy()
        for e in range(B):
            n = int(n_run[e])
            if n > 0:  # (n <= 0: the environment keeps the pair it came with)
                a_last[e], x_last[e] = acts[n - 1, e], xs[n - 1, e]
        have = pend is not None or bool((n_run > 0).any())
        self._t, self._pending = self._t + T, ((a_last, x_last) if have else None)
        if (pend is not None or T > 1) and bool((n_run == T).any()):
            self.last_bw = torch.from_numpy(bw[-1].copy())
        self.ticks += T
        res = DualSimResult(*(torch.from_numpy(np.ascontiguousarray(v)) for v in (xs, acts, pw, bw, costs, loss, status, n_run, a_seq)))
        res.t0 = t0 + T
        return res


class DualSimResult(collections.namedtuple("DualSimResult", "states actions p_weights bw costs loss status n_run a_seq")):
    """What BatchDualSVMPC.simulate returns; `t0`: the periods the episode has run so far (simulate(resume=) goes on from there)"""
    t0 = 0
