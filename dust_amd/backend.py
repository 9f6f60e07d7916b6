"""Thin object wrapper over the C ABI (one `Context` = one dust_ctx = one controller + its SVMPC state on one GPU).

All array arguments are numpy (or anything np.asarray accepts, torch CPU tensors included); results are numpy fp32.
No arithmetic of the hot path happens here - only shape checks and pointer plumbing.
"""
import ctypes as C

import numpy as np

from . import _lib as L


def _f(a, shape=None):
    a = np.ascontiguousarray(np.asarray(a, dtype=np.float32))
    if shape is not None:
        a = np.ascontiguousarray(a.reshape(shape))
    return a


def _fh(a, shape):
    """Bulk noise / action input: a float16 array stays binary16 (storage only, DUST_EPS_F16); anything else becomes fp32.
    Returns (array or None, flag)."""
    if a is None:
        return None, 0
    a = np.asarray(a)
    if a.dtype == np.float16:
        return np.ascontiguousarray(a.reshape(shape)), L.EPS_F16
    return _f(a, shape), 0


def _p(a):
    return None if a is None else a.ctypes.data_as(L.FP)


def _vp(a):
    return None if a is None else C.cast(a.ctypes.data_as(L.FP), L.VP)


# What make_config needs to know of a family: ids, (dim_a, dim_s), the action bound without min_a / max_a (None: Particle's max_accel)
# and the default dt (None: the family has none)
_FAMILIES = {
    "pendulum": dict(model=L.MODEL_PENDULUM, cost=L.COST_PENDULUM_QUADCOS, dims=(1, 2), bound=2.0, dt=0.05),
    "particle": dict(model=L.MODEL_PARTICLE, cost=L.COST_PARTICLE_DEFAULT, dims=(2, 4), bound=None, dt=0.015),
    "skid_steer": dict(model=L.MODEL_SKID_STEER, cost=L.COST_QUADRATIC, dims=(2, 5), bound=0.5, dt=None),
    "cartpole": dict(model=L.MODEL_CARTPOLE, cost=L.COST_QUADRATIC, dims=(1, 4), bound=1.0, dt=0.05),
}


def make_config(model="pendulum", N=1, S=1, M=1, H=1, uncertain_params=None, params_scalar_event=False,
                params_log_space=False, kernel="K1", likelihood="ExponentiatedUtility", optimizer="SGD", lr=1.0,
                alpha=1.0, temperature=None, ctrl_penalty=1.0, sigma_a=1.0, sigma_p=1.0, chol_a=None, a_pre=None,
                weighted_prior=False, roll_strategy="repeat", bw_scale=1.0, imq_ell=1.0, seed=0, device=0,
                shard_offset=0, shard_size=0, dt=None, g=9.8, mass=1.0, length=1.0, mass_0dim=False, w_cos=50.0, w_vel=1.0,
                max_speed=5.0, max_accel=10.0, can_crash=True, with_obstacle=True, cell_size=0.1,
                target=(9.0, 9.0, 0.0, 0.0), w_state=(0.5, 0.5, 0.25, 0.25), w_term=(1e3, 1e3, 0.1, 0.1), w_ctrl=(0.2, 0.2),
                w_obs=1e6, min_a=None, max_a=None, adam=(0.9, 0.999, 1e-8), sampling=None, control_type="acceleration",
                deterministic=True, noise_std=(0.0, 0.0), a_cov=None, p_cov=None, **_ignored):
    """a_cov / p_cov: FULL [da, da] action / prior-component covariances (MultiDISCO(a_cov=) disco.py:91-98; get_gmm svgd.py:84-89);
    they take precedence over sigma_a / sigma_p / chol_a / a_pre, which describe diagonal ones."""
    c = L.Config()
    c.abi_version = L.ABI_VERSION
    c.device = device
    if model not in _FAMILIES:
        raise ValueError("unknown model family %r" % (model,))
    fam = _FAMILIES[model]
    skid, cart, part = (model == k for k in ("skid_steer", "cartpole", "particle"))
    c.model, c.cost = fam["model"], fam["cost"]
    c.n_policies, c.n_samples, c.n_params, c.horizon = N, S, M, H
    if control_type not in ("acceleration", "velocity"):
        raise IOError('control_type "{}" not recognized'.format(control_type))  # particle.py:59-60
    vel = control_type == "velocity" and part
    c.dim_a, c.dim_s = (2, 2) if vel else fam["dims"]
    if part:  # Particle(control_type=, deterministic=, noise_std=) particle.py:13-31
        c.control_type = L.CONTROL_VELOCITY if vel else L.CONTROL_ACCELERATION
        c.ctrl_noise = int(not deterministic)
        ns = np.broadcast_to(np.asarray(noise_std, np.float32).reshape(-1), (2,))
        c.dyn_std[0], c.dyn_std[1] = float(ns[0]), float(ns[1])
    up = list(uncertain_params) if uncertain_params else []
    use_params = bool(up) if sampling is None else bool(sampling)
    c.dim_p = len(up) if use_params else 0
    c.shard_offset, c.shard_size = shard_offset, shard_size
    c.kernel = {"K1": L.KERNEL_K1_RBF, "K2": L.KERNEL_K2_IIDMP, "K2shared": L.KERNEL_K2_SHARED, "IMQ": L.KERNEL_IMQ}[kernel]
    c.likelihood = L.LIK_EXP_UTILITY if likelihood == "ExponentiatedUtility" else L.LIK_EXPECTED_COST
    c.optimizer = L.OPT_SGD if optimizer == "SGD" else L.OPT_ADAM
    c.roll_strategy = {"repeat": L.ROLL_REPEAT, "mean": L.ROLL_MEAN, "resample": L.ROLL_RESAMPLE}[roll_strategy]
    c.weighted_prior = int(weighted_prior)
    c.params_log_space = int(params_log_space)
    c.params_interleave = int(params_scalar_event)
    c.alpha = alpha
    c.temperature = (1.0 / alpha) if temperature is None else temperature
    c.a_reg = np.float32(c.temperature * (1.0 - ctrl_penalty))
    c.lr = lr
    c.adam_beta1, c.adam_beta2, c.adam_eps = adam
    sa = np.broadcast_to(np.asarray(sigma_a, np.float32), (c.dim_a,))
    sp = np.broadcast_to(np.asarray(sigma_p, np.float32), (c.dim_a,))
    ch = sa if chol_a is None else np.broadcast_to(np.asarray(chol_a, np.float32), (c.dim_a,))
    ap = (1.0 / (sa.astype(np.float32) ** 2)) if a_pre is None else np.broadcast_to(np.asarray(a_pre, np.float32), (c.dim_a,))
    for d in range(c.dim_a):
        c.sigma_a[d], c.sigma_p[d], c.chol_a[d], c.a_pre[d] = sa[d], sp[d], ch[d], ap[d]
    if a_cov is not None or p_cov is not None:
        import torch  # (the factorisations in fp32, as the reference's torch.linalg.cholesky / torch.inverse produce them)

        ac = torch.diag(torch.as_tensor(sa.astype(np.float32)) ** 2) if a_cov is None else torch.as_tensor(np.asarray(a_cov, np.float32))
        pc = torch.diag(torch.as_tensor(sp.astype(np.float32)) ** 2) if p_cov is None else torch.as_tensor(np.asarray(p_cov, np.float32))
        if tuple(ac.shape) != (c.dim_a, c.dim_a) or tuple(pc.shape) != (c.dim_a, c.dim_a):
            raise ValueError("a_cov / p_cov must be [%d, %d] matrices" % (c.dim_a, c.dim_a))
        la, lp, pre = torch.linalg.cholesky(ac), torch.linalg.cholesky(pc), torch.inverse(ac)
        for d in range(c.dim_a):
            c.chol_a[d], c.a_pre[d] = float(la[d, d]), float(pre[d, d])
            c.sigma_a[d], c.sigma_p[d] = float(ac[d, d].sqrt()), float(pc[d, d].sqrt())
        off = c.dim_a == 2 and (float(ac[0, 1]) != 0.0 or float(ac[1, 0]) != 0.0 or float(pc[0, 1]) != 0.0 or float(pc[1, 0]) != 0.0)
        if off:
            c.full_cov = 1
            c.chol_a_off, c.a_pre_off = float(la[1, 0]), float(pre[0, 1])
            c.chol_p[0], c.chol_p[1], c.chol_p[2] = float(lp[0, 0]), float(lp[1, 0]), float(lp[1, 1])
        elif c.dim_a > 2 or not torch.equal(ac, torch.diag(torch.diag(ac))) or not torch.equal(pc, torch.diag(torch.diag(pc))):
            raise NotImplementedError("full covariances are implemented for dim_a = 2")
    c.bw_scale, c.imq_ell = bw_scale, imq_ell
    bound = max_accel if fam["bound"] is None else fam["bound"]
    lo = np.broadcast_to(np.asarray(-bound if min_a is None else min_a, np.float32), (c.dim_a,))
    hi = np.broadcast_to(np.asarray(bound if max_a is None else max_a, np.float32), (c.dim_a,))
    for d in range(c.dim_a):
        c.min_a[d], c.max_a[d] = lo[d], hi[d]
    c.seed = seed
    if skid and dt is None:
        raise ValueError("SkidSteerRobot(delta_t=...) has no default: pass dt")
    c.dt = fam["dt"] if dt is None else dt

    def par(name, value):
        if use_params and name in up:
            return L.Param(L.PARAM_SAMPLED, up.index(name), float(value))
        return L.Param(L.PARAM_TENSOR0D if (mass_0dim and name == "mass") else L.PARAM_PYFLOAT, 0, float(value))

    if cart:  # (its seven parameters travel through dust_set_cartpole; the Pendulum fields stay at their defaults)
        up, g, length = [], 9.8, 1.0
    c.g, c.mass, c.length = par("g", g), par("mass", mass), par("length", length)
    c.max_torque, c.max_speed_pend, c.w_cos, c.w_vel = 2.0, 8.0, w_cos, w_vel
    c.max_speed, c.max_accel = max_speed, max_accel
    c.can_crash, c.with_obstacle = int(can_crash), int(with_obstacle and part)
    c.cell_size = cell_size
    pad4 = lambda v: (list(np.asarray(v, np.float32).reshape(-1)) + [0.0] * 4)[:4]  # (velocity control: two-entry target / weights)
    c.target[:] = pad4(target)
    c.w_state[:] = pad4(w_state)
    c.w_term[:] = pad4(w_term)
    c.w_ctrl[:] = list(w_ctrl)
    c.w_obs = w_obs
    return c


CARTPOLE_PARAMS = ("g", "f_mag", "mass_cart", "mass_pole", "length", "mu_c", "mu_p")  # CartPoleModel.__init__ order, cartpole.py:42-51


def _cartpole_struct(values, sampled):
    """dust_cartpole_config with the seven parameters: the names in `sampled` become particle / params columns in that order."""
    unknown = [k for k in sampled if k not in CARTPOLE_PARAMS]
    if unknown:
        raise ValueError("CartPoleModel has no parameter %r" % (unknown[0],))
    if len(sampled) > 4:
        raise ValueError("at most 4 uncertain parameters (dim_p <= 4), got %d" % len(sampled))
    g = L.CartPoleConfig()
    for name in CARTPOLE_PARAMS:
        v = float(values[name])
        setattr(g, name, L.Param(L.PARAM_SAMPLED, sampled.index(name), v) if name in sampled else L.Param(L.PARAM_PYFLOAT, 0, v))
    return g


class Context:
    def __init__(self, cfg=None, grid=None, _handle=None, **kw):
        self._h = None
        lib = L.load()
        k2_bw, k2_min = kw.pop("k2_bandwidth", None), kw.pop("k2_minimum_bw", 1e-5)
        optim = kw.pop("optim", None)  # dust_amd.optim.optimizer_config(...): an optimiser beyond dust_config's plain SGD / Adam
        skid_kw = {k: kw.pop(k) for k in ("x_icr", "wheel_radius", "axial_distance", "goal", "w_quad_state", "w_quad_term", "w_quad_ctrl")
                   if k in kw}
        cart_kw = {k: kw[k] for k in CARTPOLE_PARAMS if k in kw} if kw.get("model") == "cartpole" else {}
        # skid-steer: w_obs is the navigation family's obstacle weight (dust_set_obstacle_cost), not Particle's dust_config field
        nav_w_obs = kw.pop("w_obs", None) if kw.get("model") == "skid_steer" else None
        if _handle is not None:
            self._h = _handle
        else:
            self.cfg = cfg if cfg is not None else make_config(**kw)
            h = L.VP()
            L.check(lib.dust_create(C.byref(self.cfg), C.byref(h)))
            self._h = h
        got = L.Config()
        L.check(lib.dust_get_config(self._h, C.byref(got)))
        self.cfg = got
        self.N, self.S, self.M, self.H = got.n_policies, got.n_samples, got.n_params, got.horizon
        self.da, self.ds, self.P = got.dim_a, got.dim_s, got.dim_p
        self.D = self.H * self.da
        # per-tick buffers of the control loop with their ctypes pointers made ONCE: `array.ctypes.data_as(...)` costs 2.8 us per call, and
        # a closed-loop tick needs three of them - 8 us of its 19 us beyond the kernel (tools/closed_loop_probe.py)
        self._tick_state = np.zeros(self.ds, np.float32)
        self._tick_aseq = np.zeros((self.H, self.da), np.float32)
        self._tick_pw = np.zeros(self.N, np.float32)
        self._tick_ptrs = (_p(self._tick_state), _p(self._tick_aseq), _p(self._tick_pw))
        self._tick_fn = lib.dust_svmpc_tick
        if grid is not None:
            self.set_grid(grid)
        if _handle is None and got.model == L.MODEL_SKID_STEER:
            self.set_skid_steer(uncertain_params=kw.get("uncertain_params"), sampling=kw.get("sampling"), **skid_kw)
            if nav_w_obs is not None:
                self.set_obstacle_cost(nav_w_obs)
        if _handle is None and got.model == L.MODEL_CARTPOLE:
            cart_kw.update({k: v for k, v in skid_kw.items() if k in ("goal", "w_quad_state", "w_quad_term", "w_quad_ctrl")})
            self.set_cartpole(uncertain_params=kw.get("uncertain_params"), sampling=kw.get("sampling"), **cart_kw)
        # iid_mp(RBF(bandwidth >= 0)): fixed bandwidth instead of the median trick; RBF(minimum_bw=): the clamp of either (base_kernels.py:44-92)
        if (k2_bw is not None and float(k2_bw) >= 0) or (_handle is None and float(k2_min) != 1e-5 and got.kernel in (L.KERNEL_K2_IIDMP, L.KERNEL_K2_SHARED)):
            L.check(lib.dust_set_k2_bandwidth(self._h, float(-1.0 if k2_bw is None else k2_bw), float(k2_min)))
        if _handle is None and optim is not None:
            from . import optim as _optim

            if not _optim.is_plain(optim):
                self.set_optimizer(optim)

    def set_optimizer(self, optim):
        """dust_set_optimizer: the optimiser of a dict from dust_amd.optim.optimizer_config replaces the context's; its state restarts."""
        from . import optim as _optim

        L.check(L.load().dust_set_optimizer(self._h, C.byref(_optim.to_struct(optim))))

    def get_optimizer(self):
        """The context's optimiser as a dict of dust_amd.optim.optimizer_config (dust_get_optimizer)."""
        from . import optim as _optim

        o = L.OptimConfig()
        L.check(L.load().dust_get_optimizer(self._h, C.byref(o)))
        return _optim.from_struct(o)

    # ---- lifecycle
    # ---- C-side multi-GPU tick (include/dust_amd.h dust_comm_*): one RCCL communicator per sharded context
    @staticmethod
    def comm_unique_id():
        """ncclGetUniqueId on the calling rank: 128 opaque bytes to hand to every rank (e.g. torch.distributed.broadcast_object_list)."""
        buf = C.create_string_buffer(128)
        L.check(L.load().dust_comm_unique_id(C.cast(buf, L.VP)))
        return buf.raw

    def comm_validate(self, rank, world):
        """The local (non-collective) checks of comm_init; raises on failure.  Call it on every rank and let the ranks agree before comm_init."""
        L.check(L.load().dust_comm_validate(self._h, int(rank), int(world)))

    def comm_init(self, unique_id, rank, world):
        """ncclCommInitRank (collective over the ranks).  Afterwards svmpc_tick / svmpc_optimize / svmpc_forward run the sharded tick."""
        buf = C.create_string_buffer(bytes(unique_id), 128)
        L.check(L.load().dust_comm_init(self._h, C.cast(buf, L.VP), int(rank), int(world)))

    def comm_probe(self, n_steps, reps=50):
        """Microseconds per tick of the sharded tick's all-gathers alone (collective over all ranks)."""
        us = C.c_double(0.0)
        L.check(L.load().dust_comm_probe(self._h, int(n_steps), int(reps), C.byref(us)))
        return float(us.value)

    def dual_tick(self, mpf, state, action_prev, n_steps, mpf_steps=20, mpf_bw=None, seed=0, want_outputs=True):
        """One control period of the dual loop in one C call (dust_dual_tick): filter update for (action_prev, state) - skipped when
        action_prev is None -, the controller's dynamics samples drawn from the filter's refreshed prior on the device, the control
        tick.  mpf_bw None: Silverman's rule of the filter's particles, on the device.  Returns (a_seq, p_weights, bw_used)."""
        st = _f(state, (self.ds,))
        ap = None if action_prev is None else _f(action_prev).reshape(-1)
        a_seq = np.empty((self.H, self.da), np.float32) if want_outputs else None
        pw = np.empty(self.N, np.float32) if want_outputs else None
        bw = C.c_float(0.0)
        L.check(L.load().dust_dual_tick(self._h, mpf._h, _p(st), _p(ap), int(n_steps), int(mpf_steps), float(-1.0 if mpf_bw is None else mpf_bw),
                                        int(seed), _p(a_seq), _p(pw), C.cast(C.byref(bw), L.FP)))
        return a_seq, pw, float(bw.value)

    def comm_peer_gather(self, on=True):
        """The tick's all-gathers as direct peer stores through IPC-mapped buffers (collective: every rank calls it, or none)."""
        L.check(L.load().dust_comm_peer_gather(self._h, 1 if on else 0))

    def close(self):
        if self._h is not None:
            if not getattr(self, "_borrowed", False):  # (an AmppiBatch's inner context belongs to the batch)
                L.load().dust_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def clone(self):
        h = L.VP()
        L.check(L.load().dust_clone(self._h, C.byref(h)))
        return Context(_handle=h)

    def __deepcopy__(self, memo):
        return self.clone()

    def sync(self):
        L.check(L.load().dust_sync(self._h))

    def tick_stats(self):
        """Sticky counts of the device path that served optimize / tick calls: owner-computes one-launch ticks, tiled one-launch
        ticks, and ticks replayed on the launch-per-iteration path because the device was shared."""
        n = (C.c_longlong * 4)()
        L.check(L.load().dust_tick_stats(self._h, n))
        return dict(tick2=int(n[0]), tick1=int(n[1]), served=int(n[2]), replayed=int(n[3]))

    def serve_start(self, n_steps, wait_us=2000.0):
        """Closed-loop serving (dust_svmpc_serve_start): svmpc_tick(state, n_steps) calls receive their outputs through pinned host
        memory and launch the next tick ahead of its plant state (it waits at most wait_us for it).  Same results, bit for bit."""
        L.check(L.load().dust_svmpc_serve_start(self._h, int(n_steps), float(wait_us)))

    def serve_stop(self):
        L.check(L.load().dust_svmpc_serve_stop(self._h))

    def set_grid(self, grid, off=None):
        g = _f(grid)
        nx, ny = g.shape
        ox, oy = (int(nx / 2), int(ny / 2)) if off is None else off
        L.check(L.load().dust_set_grid(self._h, _p(g), nx, ny, float(ox), float(oy)))

    def set_obstacle_cost(self, w_obs):
        """The obstacle weight of a skid-steer context's cost (dust_set_obstacle_cost; dust_amd.costs.NavigationCost): w_obs occ(x, y) on
        the map of set_grid with the configuration's cell_size joins the instantaneous and the terminal cost; 0 returns to the plain kernels."""
        L.check(L.load().dust_set_obstacle_cost(self._h, float(w_obs)))

    def set_skid_steer(self, x_icr=0.2, wheel_radius=0.0625, axial_distance=0.475, goal=(0, 0, 0, 0, 0), w_quad_state=(1, 1, 1, 1, 1),
                       w_quad_term=(1, 1, 1, 1, 1), w_quad_ctrl=(0, 0), uncertain_params=None, sampling=None):
        """SkidSteerRobot parameters (skid_steer_robot.py:19-45; `uncertain_params` name the sampled ones, in column order) and the
        quadratic cost family (dust_amd.costs.QuadraticCost).  Wheel-speed bounds are the context's min_a / max_a."""
        up = list(uncertain_params) if uncertain_params else []
        use = bool(up) if sampling is None else bool(sampling)
        g = L.SkidConfig()

        def par(name, value):
            if use and name in up:
                return L.Param(L.PARAM_SAMPLED, up.index(name), float(value))
            return L.Param(L.PARAM_PYFLOAT, 0, float(value))

        g.x_icr, g.wheel_radius, g.axial_distance = par("x_icr", x_icr), par("wheel_radius", wheel_radius), par("axial_distance", axial_distance)
        for d in range(2):
            g.min_wheel_speed[d], g.max_wheel_speed[d] = self.cfg.min_a[d], self.cfg.max_a[d]
        g.goal[:] = [float(v) for v in goal]
        g.w_state[:] = [float(v) for v in w_quad_state]
        g.w_term[:] = [float(v) for v in w_quad_term]
        g.w_ctrl[:] = [float(v) for v in w_quad_ctrl]
        L.check(L.load().dust_set_skid_steer(self._h, C.byref(g)))

    def set_cartpole(self, g=9.8, f_mag=10.0, mass_cart=1.0, mass_pole=0.1, length=1.0, mu_c=0.5e-3, mu_p=2e-6, goal=(0, 0, 0, 0),
                     w_quad_state=(1, 1, 1, 1), w_quad_term=(1, 1, 1, 1), w_quad_ctrl=(0,), uncertain_params=None, sampling=None):
        """CartPoleModel parameters (cartpole.py:42-51; `uncertain_params` name the sampled ones, in column order) and the quadratic
        cost family (dust_amd.costs.QuadraticCost: 4 state entries, 1 control weight)."""
        up = list(uncertain_params) if uncertain_params else []
        use = bool(up) if sampling is None else bool(sampling)
        cfg = _cartpole_struct(dict(g=g, f_mag=f_mag, mass_cart=mass_cart, mass_pole=mass_pole, length=length, mu_c=mu_c, mu_p=mu_p), up if use else [])
        cfg.goal[:] = [float(v) for v in goal]
        cfg.w_state[:] = [float(v) for v in w_quad_state]
        cfg.w_term[:] = [float(v) for v in w_quad_term]
        cfg.w_ctrl[:] = [float(v) for v in w_quad_ctrl]
        L.check(L.load().dust_set_cartpole(self._h, C.byref(cfg)))

    def set_ctrl_noise(self, z):
        """Recorded control-channel noise for the next rollouts of a Particle(deterministic=False) context (particle.py:145-148):
        z [n_sets][H][M*S*N][da] standard-normal draws in the reference's own order (one randn_like per model.step call); None: back
        to the device Philox stream."""
        if z is None:
            L.check(L.load().dust_set_ctrl_noise(self._h, None, 0))
            return
        z = _f(z, (-1, self.H, self.M * self.S * self.N, self.da))
        L.check(L.load().dust_set_ctrl_noise(self._h, _p(z), int(z.shape[0])))

    def set_param_weights(self, w):
        """Unscented-transform weights of the n_params dynamics samples (None: plain mean)."""
        L.check(L.load().dust_set_param_weights(self._h, _p(None if w is None else _f(w, (self.M,)))))

    def set_sigma_scale(self, scale):
        """lambda + n of the transform whose weights set_param_weights set (dual_tick computes the filter's sigma points with it); 0 clears."""
        L.check(L.load().dust_set_sigma_scale(self._h, float(scale)))

    def set_model_param(self, name, value, kind=-1):
        L.check(L.load().dust_set_model_param(self._h, name.encode(), float(value), kind))

    # ---- state
    def _get(self, fn, shape):
        out = np.empty(shape, np.float32)
        L.check(fn(self._h, _p(out)))
        return out

    def set_theta(self, theta):
        L.check(L.load().dust_set_theta(self._h, _p(_f(theta, (self.N, self.H, self.da)))))

    def get_theta(self):
        return self._get(L.load().dust_get_theta, (self.N, self.H, self.da))

    def set_prior(self, means, weights=None):
        w = None if weights is None else _f(weights, (self.N,))
        L.check(L.load().dust_set_prior(self._h, _p(_f(means, (self.N, self.H, self.da))), _p(w)))

    def get_prior(self):
        means = np.empty((self.N, self.H, self.da), np.float32)
        probs = np.empty(self.N, np.float32)
        L.check(L.load().dust_get_prior(self._h, _p(means), _p(probs)))
        return means, probs

    def set_a_mat(self, a):
        L.check(L.load().dust_set_a_mat(self._h, _p(_f(a, (self.N, self.H, self.da)))))

    def get_a_mat(self):
        return self._get(L.load().dust_get_a_mat, (self.N, self.H, self.da))

    def get_a_mix(self):
        return self._get(L.load().dust_get_a_mix, (self.N,))

    def set_a_seq(self, a):
        L.check(L.load().dust_set_a_seq(self._h, _p(_f(a, (self.H, self.da)))))

    def get_a_seq(self):
        return self._get(L.load().dust_get_a_seq, (self.H, self.da))

    # ---- a1-a6
    def _params(self, params, sets=1):
        if self.P == 0:
            return None
        if params is None:
            raise ValueError("params_sampling is on: pass the sampled dynamics parameters")
        return _f(params, (sets, self.M, self.P))

    def disco_forward(self, state, actions=None, params=None, want_states=False, want_actions=False, want_omega=True,
                      around_a_mat=False, store_f16=False):
        """`actions` may be a float16 array (binary16 storage, fp32 arithmetic); `store_f16`: states / actions come back as float16."""
        st = _f(state, (self.ds,))
        act, fl = _fh(actions, (self.S, self.N, self.H, self.da))
        pr = self._params(params)
        odt = np.float16 if store_f16 else np.float32
        costs = np.empty((self.S, self.N), np.float32)
        states = np.empty((self.M, self.S, self.N, self.H + 1, self.ds), odt) if want_states else None
        aout = np.empty((self.S, self.N, self.H, self.da), odt) if want_actions else None
        omega = np.empty((self.S, self.N), np.float32) if want_omega else None
        flags = (L.EPS_AROUND_A_MAT if around_a_mat else 0) | fl | (L.STORE_F16 if store_f16 else 0)
        L.check(L.load().dust_disco_forward(self._h, _p(st), _vp(act), _p(pr), flags, _p(costs), _p(states), _p(aout), _p(omega)))
        return costs, states, (aout if aout is not None else act), omega

    def disco_step(self, strategy="argmax", steps=1, ext_actions=None):
        sid = {"argmax": L.STEP_ARGMAX, "average": L.STEP_AVERAGE, "external": L.STEP_EXTERNAL}.get(strategy, -1)
        ext = None if ext_actions is None else _f(ext_actions, (self.H, self.da))
        out = np.empty((steps, self.da), np.float32)
        L.check(L.load().dust_disco_step(self._h, sid, steps, _p(ext), _p(out)))
        return out

    def likelihood_sample(self, state, eps=None, params=None, want_actions=False, store_states=False, store_f16=False):
        st = _f(state, (self.ds,))
        e, fl = _fh(eps, (self.S, self.N, self.H, self.da))
        pr = self._params(params)
        costs = np.empty((self.S, self.N), np.float32)
        aout = np.empty((self.S, self.N, self.H, self.da), np.float16 if store_f16 else np.float32) if want_actions else None
        flags = (L.STORE_STATES if store_states else 0) | fl | (L.STORE_F16 if store_f16 else 0)
        L.check(L.load().dust_likelihood_sample(self._h, _p(st), _vp(e), _p(pr), flags, _p(costs), _p(aout)))
        return (costs, aout) if want_actions else costs

    def likelihood_log_prob(self):
        return self._get(L.load().dust_likelihood_log_prob, (self.N,))

    # ---- a7-a12
    def svmpc_phi(self, costs=None, actions=None):
        c = None if costs is None else _f(costs, (self.S, self.N))
        a = None if actions is None else _f(actions, (self.S, self.N, self.H, self.da))
        phi, gl, gp = (np.empty((self.N, self.H, self.da), np.float32) for _ in range(3))
        L.check(L.load().dust_svmpc_phi(self._h, _p(c), _p(a), _p(phi), _p(gl), _p(gp)))
        return phi, gl, gp

    def svmpc_optimize(self, state, n_steps, eps=None, params=None):
        st = _f(state, (self.ds,))
        e, fl = _fh(eps, (n_steps, self.S, self.N, self.H, self.da))
        pr = self._params(params, n_steps)
        L.check(L.load().dust_svmpc_optimize(self._h, _p(st), n_steps, _vp(e), _p(pr), fl))

    def svmpc_optimize_dev(self, state, n_steps, eps_dev_ptr, params=None):
        st = _f(state, (self.ds,))
        pr = self._params(params, n_steps)
        L.check(L.load().dust_svmpc_optimize(self._h, _p(st), n_steps, L.VP(eps_dev_ptr) if eps_dev_ptr else None, _p(pr),
                                             L.PTR_DEVICE))

    def svmpc_forward(self):
        a_seq = np.empty((self.H, self.da), np.float32)
        pw = np.empty(self.N, np.float32)
        L.check(L.load().dust_svmpc_forward(self._h, _p(a_seq), _p(pw)))
        return a_seq, pw

    def likelihood_sample_at(self, state, theta, eps=None, params=None, want_actions=False):
        """CostLikelihood.sample(theta, ...) for a theta that is not the optimiser's: the context's particles / Adam state stay."""
        st = _f(state, (self.ds,))
        th = _f(theta, (self.N, self.H, self.da))
        e, fl = _fh(eps, (self.S, self.N, self.H, self.da))
        pr = self._params(params)
        costs = np.empty((self.S, self.N), np.float32)
        aout = np.empty((self.S, self.N, self.H, self.da), np.float32) if want_actions else None
        L.check(L.load().dust_likelihood_sample_at(self._h, _p(st), _p(th), _vp(e), _p(pr), fl, _p(costs), _p(aout)))
        return (costs, aout) if want_actions else costs

    def svmpc_get_weights(self):
        pw = np.empty(self.N, np.float32)
        L.check(L.load().dust_svmpc_get_weights(self._h, _p(pw)))
        return pw

    def svmpc_roll(self, steps=-1, strategy="repeat", last_row=None):
        st = {"repeat": L.ROLL_REPEAT, "mean": L.ROLL_MEAN, "resample": L.ROLL_RESAMPLE}.get(strategy)
        if st is None:
            raise ValueError("{} is an invalid roll strategy.".format(strategy))
        lr = None if last_row is None else _f(last_row, (self.N, self.da))
        L.check(L.load().dust_svmpc_roll(self._h, int(steps), st, _p(lr)))

    def svmpc_update_prior(self, weights=None):
        w = None if weights is None else _f(weights, (self.N,))
        L.check(L.load().dust_svmpc_update_prior(self._h, _p(w)))

    def svmpc_forward_ex(self, steps=-1, resample_last_row=None):
        a_seq, pw = np.empty((self.H, self.da), np.float32), np.empty(self.N, np.float32)
        lr = None if resample_last_row is None else _f(resample_last_row, (self.N, self.da))
        L.check(L.load().dust_svmpc_forward_ex(self._h, int(steps), _p(lr), _p(a_seq), _p(pw)))
        return a_seq, pw

    def svmpc_tick(self, state, n_steps, eps=None, params=None, eps_dev_ptr=None, want_outputs=True):
        if eps is None and params is None and not eps_dev_ptr and self.P == 0:
            # the control loop's call (device noise, nominal dynamics): cached buffers and pointers, the outputs handed back as copies
            self._tick_state[:] = np.asarray(state, np.float32).reshape(self.ds)
            ps, pa, pw_ = self._tick_ptrs
            if want_outputs == "action":  # the chosen sequence only (what a control loop sends to its plant): p_weights are not fetched
                L.check(self._tick_fn(self._h, ps, n_steps, None, None, 0, pa, None))
                return self._tick_aseq.copy(), None
            if want_outputs:
                L.check(self._tick_fn(self._h, ps, n_steps, None, None, 0, pa, pw_))
                return self._tick_aseq.copy(), self._tick_pw.copy()
            L.check(self._tick_fn(self._h, ps, n_steps, None, None, 0, None, None))
            return None, None
        st = _f(state, (self.ds,))
        pr = self._params(params, n_steps)
        a_seq = np.empty((self.H, self.da), np.float32) if want_outputs else None
        pw = np.empty(self.N, np.float32) if want_outputs and want_outputs != "action" else None
        if eps_dev_ptr:
            e, flags = L.VP(eps_dev_ptr), L.PTR_DEVICE
        else:
            e, flags = _fh(eps, (n_steps, self.S, self.N, self.H, self.da))
            e = _vp(e)
        L.check(L.load().dust_svmpc_tick(self._h, _p(st), n_steps, e, _p(pr), flags, _p(a_seq), _p(pw)))
        return a_seq, pw

    # ---- AMPPI (amppi.py:227-260, base.py:68-80)
    def amppi_update(self, state, actions=None, params=None, shared_params=False, want_states=False, want_actions=False, want_outputs=True):
        """One AMPPI.update_actions tick (dust_amppi_update).  actions [S, H, da] or None (drawn on the device); params None ("none"),
        one row with shared_params ("single"), [S, P] ("extended") or the [2P + 1, P] sigma points of a context with parameter weights.
        -> (costs [S], omega [S], a_seq [H, da] after the update, states [S pts, H + 1, ds] or None, acts [S, H, da] or None);
        want_outputs=False reads nothing back (the tick stays asynchronous on the context's stream)."""
        st = _f(state, (self.ds,))
        act = None if actions is None else _f(actions, (self.S, self.H, self.da))
        pr = None if params is None else _f(params, (-1, max(self.P, 1)))  # (rows for a context without uncertain parameters: the library refuses)
        pts = self.M  # (an AMPPI context has n_params > 1 only as the 2P + 1 sigma points: the library refuses it without their weights)
        want_rows = None if pr is None else (pts if pts > 1 else (1 if shared_params else self.S))
        if pr is not None and pr.shape[0] < want_rows:
            raise ValueError("params has %d rows, the tick reads %d" % (pr.shape[0], want_rows))
        if pr is not None and shared_params:
            pr = pr[:1].copy()
        flags = (L.AMPPI_PARAMS_SHARED if shared_params else 0) | (L.STORE_STATES if want_states else 0)
        costs, omega, a_seq = ((np.empty(self.S, np.float32), np.empty(self.S, np.float32), np.empty((self.H, self.da), np.float32))
                               if want_outputs else (None, None, None))
        L.check(L.load().dust_amppi_update(self._h, _p(st), _vp(act), _p(pr), flags, _p(costs), _p(omega), _p(a_seq)))
        states = acts = None
        if want_states:
            states = self.get_states_rows(np.arange(self.S * pts))
        if want_actions:
            acts = self._get(L.load().dust_get_actions, (self.S, self.H, self.da))
        return costs, omega, a_seq, states, acts

    def amppi_dual_tick(self, mpf, state, action_prev=None, actions=None, shared_params=False, mpf_steps=20, mpf_bw=None, seed=0, roll=0,
                        want_outputs=True, want_params=False):
        """One control period of the dual loop over an AMPPI context in one C call (dust_amppi_dual_tick): the filter update for
        (action_prev, state) - skipped when action_prev is None -, the parameters from the refreshed prior (drawn inside the tick's
        kernel; one staged row with shared_params; staged sigma points for a context with parameter weights and a sigma scale), the
        update, the roll.  -> (costs [S], omega [S], a_seq [H, da] before the roll, params or None, bw_used); want_outputs=False
        reads nothing back."""
        st = _f(state, (self.ds,))
        ap = None if action_prev is None else _f(action_prev).reshape(-1)
        act = None if actions is None else _f(actions, (self.S, self.H, self.da))
        costs, omega, a_seq = ((np.empty(self.S, np.float32), np.empty(self.S, np.float32), np.empty((self.H, self.da), np.float32))
                               if want_outputs else (None, None, None))
        rows = self.M if self.M > 1 else (1 if shared_params else self.S)
        pout = np.empty((rows, max(self.P, 1)), np.float32) if want_params else None
        bw = C.c_float(0.0)
        L.check(L.load().dust_amppi_dual_tick(self._h, mpf._h, _p(st), _p(ap), _vp(act), L.AMPPI_PARAMS_SHARED if shared_params else 0,
                                              int(mpf_steps), float(-1.0 if mpf_bw is None else mpf_bw), int(seed), int(roll), _p(costs),
                                              _p(omega), _p(a_seq), _p(pout), C.cast(C.byref(bw), L.FP)))
        return costs, omega, a_seq, pout, float(bw.value)

    def amppi_roll(self, steps=1):
        """BaseController.roll(steps): the sequence moves `steps` rows forward, zeros behind (dust_amppi_roll)."""
        L.check(L.load().dust_amppi_roll(self._h, int(steps)))

    def amppi_batch(self, n_envs, seeds=None):
        """`n_envs` independent AMPPI controllers of this context's configuration, one kernel launch per tick (dust_amppi_batch_create):
        the batch keeps its own copy of the context.  seeds [n_envs] (None: this context's seed + b)."""
        return AmppiBatch(self, n_envs, seeds)

    def svmpc_batch(self, n_envs, seeds=None):
        """`n_envs` independent SVMPC controllers of this context's configuration - particles, prior, a_mat, optimiser state and noise
        stream each -, one kernel launch per optimize / forward / tick (dust_svmpc_batch_create): the batch keeps its own copy of the
        context.  seeds [n_envs] (None: this context's seed + b).  A skid-steer context with an obstacle weight (set_obstacle_cost)
        runs the navigation instance on its one map (set_grid; without a map: ERR_STATE)."""
        return SvmpcBatch(self, n_envs, seeds)

    def disco_batch(self, n_envs, seeds=None):
        """`n_envs` independent MultiDISCO controllers of this context's configuration - a_mat, a_seq, a_mix and noise stream each -, one
        kernel launch per forward / step / tick and per closed-loop episode (dust_disco_batch_create): the batch keeps its own copy of
        the context.  seeds [n_envs] (None: this context's seed + b).  Sigma-point weights (set_param_weights) make it the "DISCO" case."""
        return DiscoBatch(self, n_envs, seeds)

    def get_costs(self):
        return self._get(L.load().dust_get_costs, (self.S, self.N))

    def get_states_rows(self, rows, f16=False):
        """Trajectories [len(rows)][H+1][ds] of the states the last stored-states sample left on the device; rows = (m*S + s)*N + n."""
        r = np.ascontiguousarray(np.asarray(rows, np.int64).reshape(-1))
        out = np.empty((r.size, self.H + 1, self.ds), np.float16 if f16 else np.float32)
        L.check(L.load().dust_get_states_rows(self._h, r.ctypes.data_as(C.POINTER(C.c_longlong)), int(r.size), C.c_void_p(out.ctypes.data)))
        return out

    def get_score(self):
        return self._get(L.load().dust_get_score, (self.N, self.H, self.da))

    def get_phi(self):
        return self._get(L.load().dust_get_phi, (self.N, self.H, self.da))

    def get_score_parts(self):
        """(grad_lik, grad_pri) of the last SVGD iteration (svmpc.py:38-53)."""
        gl, gp = (np.empty((self.N, self.H, self.da), np.float32) for _ in range(2))
        L.check(L.load().dust_get_score_parts(self._h, _p(gl), _p(gp)))
        return gl, gp

    def get_log_weights(self):
        ll, lp = np.empty(self.N, np.float32), np.empty(self.N, np.float32)
        L.check(L.load().dust_get_log_weights(self._h, _p(ll), _p(lp)))
        return ll, lp

    def get_bandwidths(self):
        G = self.H if self.cfg.kernel == L.KERNEL_K2_SHARED else self.D
        return self._get(L.load().dust_get_bandwidths, (G,))

    # ---- timing
    def profile(self, on=True):
        L.check(L.load().dust_profile_enable(self._h, int(on)))
        L.check(L.load().dust_profile_reset(self._h))

    def profile_get(self):
        out = {}
        for k in range(L.K_ALL):
            ms, n = C.c_double(0), C.c_int64(0)
            L.check(L.load().dust_profile_get(self._h, k, C.byref(ms), C.byref(n)))
            if n.value:
                out[L.load().dust_kernel_name(k).decode()] = (ms.value, n.value)
        return out

    def profile_rollout(self, state, eps_dev, n_slices, reps, f16=False, store_states=False, store_f16=False):
        """Average launch-to-launch time (ms) of the standalone rollout kernel over device-resident eps slices
        (store_states: the HBM-bound form that also writes states [M][S][N][H+1][ds])."""
        ms = C.c_double(0)
        fl = (L.EPS_F16 if f16 else 0) | (L.STORE_STATES if store_states else 0) | (L.STORE_F16 if store_f16 else 0)
        L.check(L.load().dust_profile_rollout(self._h, _p(np.ascontiguousarray(state, np.float32)), C.c_void_p(eps_dev), int(n_slices),
                                              int(reps), fl, C.byref(ms)))
        return ms.value

    def rollout_bytes(self, store_states=False, eps_f16=False, store_f16=False):
        b = C.c_double(0)
        fl = (L.STORE_STATES if store_states else 0) | (L.EPS_F16 if eps_f16 else 0) | (L.STORE_F16 if store_f16 else 0)
        L.check(L.load().dust_rollout_algorithmic_bytes(self._h, fl, C.byref(b)))
        return b.value

    def device_noise(self, n_values, seed=1, f16=False):
        p = L.VP()
        L.check(L.load().dust_device_noise_alloc(self._h, n_values, seed, L.EPS_F16 if f16 else 0, C.byref(p)))
        return p.value

    def device_free(self, ptr):
        L.check(L.load().dust_device_free(self._h, L.VP(ptr)))


def _mask(active, B):
    """the active mask as [B] bytes (None: everybody) -> (array or None, ctypes pointer or None)"""
    if active is None:
        return None, None
    m = np.ascontiguousarray(np.asarray(active).reshape(-1) != 0, dtype=np.uint8)
    if m.shape != (B,):
        raise ValueError("active has %d entries, the batch has %d environments" % (m.size, B))
    return m, m.ctypes.data_as(C.POINTER(C.c_ubyte))


def _seeds(seeds, B):
    """the environments' Philox keys as [B] uint64 (None: the library's default) -> (array or None, ctypes pointer or None)"""
    if seeds is None:
        return None, None
    sd = np.ascontiguousarray(np.asarray(seeds, dtype=np.uint64).reshape(-1))
    if sd.size != B:
        raise ValueError("seeds has %d entries for %d environments" % (sd.size, B))
    return sd, sd.ctypes.data_as(C.POINTER(C.c_uint64))


def _period_seeds(seeds, rows, B):
    """an episode's Philox keys [rows, B], period by period (None: the library refuses) -> as _seeds"""
    if seeds is not None and np.shape(seeds) != (rows, B):
        raise ValueError("seeds has shape %s, the call reads %s" % (np.shape(seeds), (rows, B)))
    return _seeds(seeds, rows * B)


def _plant_rows(pl, B, P):
    """the plants' true parameter rows as [B, P] float32 (None: nominal plants)"""
    if pl is None:
        return None
    pl = _f(pl)
    if pl.shape != (B, max(P, 1)):
        raise ValueError("plant_params has shape %s, the call reads %s" % (pl.shape, (B, max(P, 1))))
    return pl


def _episode_rules(ds, t0, warm_up, goal, goal_radius, stop_on_crash):
    """the reference's episode rules as the library reads them (goal [ds] or None, goal_radius None: no goal)"""
    ru = L.EpisodeRules()
    ru.t0, ru.warm_up, ru.stop_on_crash = int(t0), int(warm_up), int(bool(stop_on_crash))
    ru.goal_radius = 0.0 if goal_radius is None else float(goal_radius)
    if goal is not None:
        g = np.asarray(goal, np.float32).reshape(-1)
        if g.shape != (ds,):
            raise ValueError("goal has %d entries, a state has %d" % (g.size, ds))
        ru.goal[:ds] = [float(v) for v in g]
    return ru


def _rules_state(B, loss, status):
    """what an episode under rules carries from call to call: loss / status [B] where a previous call left them (None: 0), and n_run
    [B] = -1 for the call to write -> (loss, status, n_run, the pointer type of the two int arrays)"""
    loss = np.zeros(B, np.float32) if loss is None else np.array(_f(loss, (B,)))
    status = np.zeros(B, np.int32) if status is None else np.ascontiguousarray(np.array(status, np.int32).reshape(B))
    return loss, status, np.full(B, -1, np.int32), C.POINTER(C.c_int)


class _BatchHandle:
    """The lifetime of a batch's C handle `_h`; a class names its library symbols in `_destroy` and `_clone`.  A controller batch's
    borrowed inner context `ctx` is closed ahead of the handle."""

    _destroy = _clone = None

    def close(self):
        if getattr(self, "_h", None) is not None:
            if getattr(self, "ctx", None) is not None:
                self.ctx.close()
            getattr(L.load(), self._destroy)(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def clone(self):
        h = L.VP()
        L.check(getattr(L.load(), self._clone)(self._h, C.byref(h)))
        return type(self)(self, n_envs=self.B, _handle=h)  # (the source in the prototype's place: a filter batch reads its sizes there)

    def __deepcopy__(self, memo):
        return self.clone()


class AmppiBatch(_BatchHandle):
    """B independent AMPPI ticks in one launch (dust_amppi_batch_*): per environment a state, a nominal sequence, a noise stream and
    parameter rows; model, cost, horizon, S, lambda and a_cov are the prototype context's.  `ctx` is the batch's inner context
    (borrowed) for sync() and profile() / profile_get()."""

    _destroy, _clone = "dust_amppi_batch_destroy", "dust_amppi_batch_clone"

    def __init__(self, proto=None, n_envs=1, seeds=None, _handle=None):
        self._h = None
        lib = L.load()
        if _handle is None:
            sd, sp = _seeds(seeds, int(n_envs))
            h = L.VP()
            L.check(lib.dust_amppi_batch_create(proto._h, int(n_envs), sp, C.byref(h)))
            _handle = h
        self._h = _handle
        self.B = int(n_envs)
        inner = L.VP()
        L.check(lib.dust_amppi_batch_ctx(self._h, C.byref(inner)))
        self.ctx = Context(_handle=inner)
        self.ctx._borrowed = True
        c = self.ctx
        self.S, self.H, self.da, self.ds, self.P, self.M = c.S, c.H, c.da, c.ds, c.P, c.M

    def set_a_seq(self, a):
        L.check(L.load().dust_amppi_batch_set_a_seq(self._h, _p(_f(a, (self.B, self.H, self.da)))))

    def get_a_seq(self):
        out = np.empty((self.B, self.H, self.da), np.float32)
        L.check(L.load().dust_amppi_batch_get_a_seq(self._h, _p(out)))
        return out

    def update(self, states, actions=None, params=None, shared_params=False, active=None, want_actions=False, want_outputs=True, flags=0,
               want_costs=True):
        """One tick of every active environment (dust_amppi_batch_update).  states [B, ds]; actions [B, S, H, da] or None (drawn on the
        device); params None ("none"), [B, 1, P] with shared_params ("single"), [B, S, P] ("extended") or [B, 2P + 1, P] sigma points;
        active [B] or None.  -> (costs [B, S], omega [B, S], a_seq [B, H, da] after the update, acts [B, S, H, da] or None); the rows of
        inactive environments are NaN.  want_outputs=False reads nothing back (the tick stays asynchronous on the batch's stream);
        want_costs=False reads a_seq alone back (costs and omega come back as None)."""
        B, S = self.B, self.S
        st = None if states is None else _f(states, (B, self.ds))  # (None: the library refuses)
        act = None if actions is None else _f(actions, (B, S, self.H, self.da))
        pr = None
        if params is not None:
            rows = self.M if self.M > 1 else (1 if shared_params else S)
            pr = _f(params)
            if pr.ndim != 3 or pr.shape[0] != B or pr.shape[1] != rows or pr.shape[2] != max(self.P, 1):
                raise ValueError("params has shape %s, the tick reads [%d, %d, %d]" % (pr.shape, B, rows, max(self.P, 1)))
        m, mp = _mask(active, B)
        fl = int(flags) | (L.AMPPI_PARAMS_SHARED if shared_params else 0)
        costs = omega = a_seq = None
        if want_outputs:
            a_seq = np.full((B, self.H, self.da), np.nan, np.float32)
            if want_costs:
                costs, omega = (np.full((B, S), np.nan, np.float32) for _ in range(2))
        L.check(L.load().dust_amppi_batch_update(self._h, _p(st), _vp(act), _p(pr), fl, mp, _p(costs), _p(omega), _p(a_seq)))
        return costs, omega, a_seq, (self.get_actions() if want_actions else None)

    def dual_tick(self, mpf, states, actions_prev=None, actions=None, shared_params=False, mpf_steps=20, mpf_bw=None, seeds=None, roll=0,
                  active=None, want_outputs=True, want_params=False, flags=0):
        """One control period of the dual loop for every active environment in one C call (dust_amppi_dual_batch_tick): the filters'
        update for (actions_prev[b], states[b]) - skipped when actions_prev is None -, the parameters from every refreshed prior (drawn
        inside the tick's kernel; one staged row per environment with shared_params; staged sigma points for a context with parameter
        weights and a sigma scale), the update, the roll.  mpf: an `MpfBatch` of B environments; seeds [B]: the Philox key of every
        environment's draws.  -> (costs [B, S], omega [B, S], a_seq [B, H, da] before the roll, params or None, bw_used [B]); the rows
        of inactive environments are NaN.  want_outputs=False reads nothing back: the call does not wait for the device."""
        B, S = self.B, self.S
        st = None if states is None else _f(states, (B, self.ds))
        ap = None if actions_prev is None else _f(actions_prev, (B, self.da))
        act = None if actions is None else _f(actions, (B, S, self.H, self.da))
        sd, sp = _seeds(seeds, B)
        _, mp = _mask(active, B)
        costs = omega = a_seq = bw = None
        if want_outputs:
            costs, omega, a_seq, bw = (np.full(sh, np.nan, np.float32) for sh in ((B, S), (B, S), (B, self.H, self.da), (B,)))
        rows = self.M if self.M > 1 else (1 if shared_params else S)
        pout = np.full((B, rows, max(self.P, 1)), np.nan, np.float32) if want_params else None
        L.check(L.load().dust_amppi_dual_batch_tick(self._h, mpf._h, _p(st), _p(ap), _vp(act), int(flags) | (L.AMPPI_PARAMS_SHARED if shared_params else 0),
                                                    int(mpf_steps), float(-1.0 if mpf_bw is None else mpf_bw), sp, int(roll), mp,
                                                    _p(costs), _p(omega), _p(a_seq), _p(pout), _p(bw)))
        return costs, omega, a_seq, pout, bw

    def get_actions(self):
        """[B, S, H, da] actions of the last tick; NaN rows for the environments that were inactive in it."""
        out = np.full((self.B, self.S, self.H, self.da), np.nan, np.float32)
        L.check(L.load().dust_amppi_batch_get_actions(self._h, _p(out)))
        return out

    def roll(self, steps=1, active=None):
        """BaseController.roll(steps) of every active environment in one launch (dust_amppi_batch_roll)."""
        _, mp = _mask(active, self.B)
        L.check(L.load().dust_amppi_batch_roll(self._h, int(steps), mp))

    def episode(self, states, n_periods, params=None, shared_params=False, plant_params=None, active=None, roll_steps=1, want_costs=True,
                flags=0):
        """n_periods closed-loop periods of every active environment with the plants on the device (dust_amppi_batch_episode): per
        period one launch - the tick (noise drawn on the device), the plant's step with the first action of the updated sequence under
        the environment's true parameters, the records, the roll - and no host between two periods.  states [B, ds]; params None,
        [T, B, 1, P] with shared_params, [T, B, S, P] or [T, B, 2P + 1, P] sigma points; plant_params [B, P] or None (nominal plants).
        -> (states [T, B, ds] after every step, actions [T, B, da], costs [T, B, S] or None, omega [T, B, S] or None, a_seq [B, H, da] of
        the last period before its roll); the rows of inactive environments are NaN."""
        B, T, S = self.B, int(n_periods), self.S
        st = None if states is None else _f(states, (B, self.ds))  # (None: the library refuses)
        pr = None
        if params is not None:
            pr = _f(params)
            want = (T, B, self.M if self.M > 1 else (1 if shared_params else S), max(self.P, 1))
            if pr.shape != want:
                raise ValueError("params has shape %s, the call reads %s" % (pr.shape, want))
        pl = _plant_rows(plant_params, B, self.P)
        _, mp = _mask(active, B)
        rows = max(T, 0)  # (n_periods < 1: the library refuses before it writes anything)
        xs, acts, a_seq = (np.full(sh, np.nan, np.float32) for sh in ((rows, B, self.ds), (rows, B, self.da), (B, self.H, self.da)))
        costs, omega = ((np.full((rows, B, S), np.nan, np.float32) for _ in range(2)) if want_costs else (None, None))
        fl = int(flags) | (L.AMPPI_PARAMS_SHARED if shared_params else 0)
        L.check(L.load().dust_amppi_batch_episode(self._h, _p(st), T, _p(pr), fl, int(roll_steps), _p(pl), mp, _p(xs), _p(acts), _p(costs),
                                                  _p(omega), _p(a_seq)))
        return xs, acts, costs, omega, a_seq

    def dual_episode(self, mpf, states, n_periods, actions_prev=None, shared_params=False, mpf_steps=20, mpf_bw=None, seeds=None, roll_steps=1,
                     plant_params=None, active=None, want_costs=True):
        """n_periods control periods of the dual loop for every active environment in one C call (dust_amppi_dual_batch_episode): per
        period the filters' update - in period 0 only with actions_prev -, the tick with its parameters from the refreshed priors and
        device-drawn noise, the plant's step with the first action of the updated sequence under the environment's true parameters,
        the roll; no host round trip between periods.  states [B, ds]; seeds [T, B]: period t's Philox keys; plant_params [B, P] or
        None (nominal plants).  -> (states [T, B, ds] after every step, actions [T, B, da], costs [T, B, S] or None, omega [T, B, S] or
        None, bw [T, B], a_seq [B, H, da] of the last period before its roll); the rows of inactive environments are NaN.  The pair
        (actions[-1], states[-1]) is still to be folded into the filters: hand it to the next call."""
        B, T, S = self.B, int(n_periods), self.S
        st = None if states is None else _f(states, (B, self.ds))  # (None: the library refuses)
        ap = None if actions_prev is None else _f(actions_prev, (B, self.da))
        rows = max(T, 0)  # (n_periods < 1: the library refuses before it reads or writes anything)
        sd, sp = _period_seeds(seeds, rows, B)
        pl = _plant_rows(plant_params, B, self.P)
        _, mp = _mask(active, B)
        xs, acts, bw, a_seq = (np.full(sh, np.nan, np.float32) for sh in ((rows, B, self.ds), (rows, B, self.da), (rows, B), (B, self.H, self.da)))
        costs, omega = ((np.full((rows, B, S), np.nan, np.float32) for _ in range(2)) if want_costs else (None, None))
        L.check(L.load().dust_amppi_dual_batch_episode(self._h, mpf._h, _p(st), _p(ap), T, L.AMPPI_PARAMS_SHARED if shared_params else 0, int(mpf_steps),
                                                       float(-1.0 if mpf_bw is None else mpf_bw), sp, int(roll_steps), _p(pl), mp,
                                                       _p(xs), _p(acts), _p(costs), _p(omega), _p(bw), _p(a_seq)))
        return xs, acts, costs, omega, bw, a_seq

    def simulate(self, states, n_periods, params=None, shared_params=False, plant_params=None, t0=0, goal=None, goal_radius=None,
                 stop_on_crash=False, loss=None, status=None, active=None, roll_steps=1, want_costs=True, flags=0, warm_up=0):
        """episode() under the reference's episode rules (dust_amppi_batch_simulate), still one launch per period and no host between two
        periods.  Period t is period t0 + t of the episode; this branch of the reference has no warm-up (warm_up != 0: the library
        refuses).  The family's instantaneous cost of every new state goes to `inst_costs` and, as an fp32 running sum, to `loss`; with
        stop_on_crash a new position on an occupied cell ends the environment with loss = inf, status 2; with goal [ds] and
        goal_radius > 0, |goal - x|^2 <= radius^2 ends it with status 1.  loss / status [B]: where a previous call left them (None: 0).
        -> (states [T, B, ds], actions [T, B, da], costs [T, B, S] or None, omega [T, B, S] or None, inst_costs [T, B], loss [B],
        status [B] int32, n_run [B] int32, a_seq [B, H, da] of every environment's last period before its roll); rows the call did not
        write - past n_run[b], inactive environments - are NaN (n_run: -1)."""
        B, T, S = self.B, int(n_periods), self.S
        st = None if states is None else _f(states, (B, self.ds))  # (None: the library refuses)
        pr = None
        if params is not None:
            pr = _f(params)
            want = (T, B, self.M if self.M > 1 else (1 if shared_params else S), max(self.P, 1))
            if pr.shape != want:
                raise ValueError("params has shape %s, the call reads %s" % (pr.shape, want))
        pl = _plant_rows(plant_params, B, self.P)
        ru = _episode_rules(self.ds, t0, warm_up, goal, goal_radius, stop_on_crash)
        _, mp = _mask(active, B)
        rows = max(T, 0)  # (n_periods < 1: the library refuses before it writes anything)
        xs, acts, ic, a_seq = (np.full(sh, np.nan, np.float32) for sh in ((rows, B, self.ds), (rows, B, self.da), (rows, B), (B, self.H, self.da)))
        costs, omega = ((np.full((rows, B, S), np.nan, np.float32) for _ in range(2)) if want_costs else (None, None))
        loss, status, n_run, IP = _rules_state(B, loss, status)
        fl = int(flags) | (L.AMPPI_PARAMS_SHARED if shared_params else 0)
        L.check(L.load().dust_amppi_batch_simulate(self._h, _p(st), T, _p(pr), fl, int(roll_steps), _p(pl), C.byref(ru), mp, _p(xs), _p(acts),
                                                   _p(costs), _p(omega), _p(ic), _p(loss), status.ctypes.data_as(IP), n_run.ctypes.data_as(IP),
                                                   _p(a_seq)))
        return xs, acts, costs, omega, ic, loss, status, n_run, a_seq

    def dual_simulate(self, mpf, states, n_periods, actions_prev=None, shared_params=False, mpf_steps=20, mpf_bw=None, seeds=None, roll_steps=1,
                      plant_params=None, t0=0, goal=None, goal_radius=None, stop_on_crash=False, loss=None, status=None, active=None,
                      want_costs=True, flags=0, warm_up=0):
        """dual_episode() under the reference's episode rules, in one C call (dust_amppi_dual_batch_simulate): the cost of every new state
        goes to `inst_costs` and, as an fp32 running sum, to `loss`; crash (status 2, loss inf) and goal (status 1) stop an environment
        on both sides - no further filter update, no tick -, and its pair (a_{n-1}, x_n) stays pending.  No warm-up.  loss / status [B]:
        where a previous call left them.  -> (states [T, B, ds], actions [T, B, da], costs [T, B, S] or None, omega [T, B, S] or None,
        bw [T, B], inst_costs [T, B], loss [B], status [B] int32, n_run [B] int32, a_seq [B, H, da]); rows the call did not write - past
        n_run[b], inactive environments - are NaN (n_run: -1)."""
        B, T, S = self.B, int(n_periods), self.S
        st = None if states is None else _f(states, (B, self.ds))  # (None: the library refuses)
        ap = None if actions_prev is None else _f(actions_prev, (B, self.da))
        rows = max(T, 0)  # (n_periods < 1: the library refuses before it reads or writes anything)
        sd, sp = _period_seeds(seeds, rows, B)
        pl = _plant_rows(plant_params, B, self.P)
        ru = _episode_rules(self.ds, t0, warm_up, goal, goal_radius, stop_on_crash)
        _, mp = _mask(active, B)
        xs, acts, bw, ic, a_seq = (np.full(sh, np.nan, np.float32)
                                   for sh in ((rows, B, self.ds), (rows, B, self.da), (rows, B), (rows, B), (B, self.H, self.da)))
        costs, omega = ((np.full((rows, B, S), np.nan, np.float32) for _ in range(2)) if want_costs else (None, None))
        loss, status, n_run, IP = _rules_state(B, loss, status)
        fl = int(flags) | (L.AMPPI_PARAMS_SHARED if shared_params else 0)
        L.check(L.load().dust_amppi_dual_batch_simulate(self._h, mpf._h, _p(st), _p(ap), T, fl, int(mpf_steps),
                                                        float(-1.0 if mpf_bw is None else mpf_bw), sp, int(roll_steps), _p(pl), C.byref(ru), mp,
                                                        _p(xs), _p(acts), _p(costs), _p(omega), _p(bw), _p(ic), _p(loss),
                                                        status.ctypes.data_as(IP), n_run.ctypes.data_as(IP), _p(a_seq)))
        return xs, acts, costs, omega, bw, ic, loss, status, n_run, a_seq


class SvmpcBatch(_BatchHandle):
    """B independent SVMPC ticks in one launch (dust_svmpc_batch_*): per environment a state, particles, a prior, a_mat, optimiser
    state, a noise stream and dynamics samples; everything else is the prototype context's.  `ctx` is the batch's inner context
    (borrowed) for sync() and profile() / profile_get()."""

    _destroy, _clone = "dust_svmpc_batch_destroy", "dust_svmpc_batch_clone"

    def __init__(self, proto=None, n_envs=1, seeds=None, _handle=None):
        self._h = None
        lib = L.load()
        if _handle is None:
            sd, sp = _seeds(seeds, int(n_envs))
            h = L.VP()
            L.check(lib.dust_svmpc_batch_create(proto._h, int(n_envs), sp, C.byref(h)))
            _handle = h
        self._h = _handle
        self.B = int(n_envs)
        inner = L.VP()
        L.check(lib.dust_svmpc_batch_ctx(self._h, C.byref(inner)))
        self.ctx = Context(_handle=inner)
        self.ctx._borrowed = True
        c = self.ctx
        self.N, self.S, self.H, self.da, self.ds, self.P, self.M = c.N, c.S, c.H, c.da, c.ds, c.P, c.M
        B, N, S, H, da = self.B, self.N, self.S, self.H, self.da
        self._hist_x_row = None  # (Mp, P) of the filters the last dual_simulate() ran with: a recorded filter row's shape
        self._shapes = {L.SVB_THETA: (B, N, H, da), L.SVB_PRIOR_MEANS: (B, N, H, da), L.SVB_PRIOR_MIX: (B, N), L.SVB_A_MAT: (B, N, H, da),
                        L.SVB_COSTS: (B, S, N), L.SVB_SCORE: (B, N, H, da), L.SVB_PHI: (B, N, H, da), L.SVB_LOG_L: (B, N),
                        L.SVB_LOG_P: (B, N), L.SVB_A_MIX: (B, N), L.SVB_ACTIONS: (B, S, N, H, da)}

    def set(self, what, value):
        """THETA / PRIOR_MEANS / A_MAT [B, N, H, da], PRIOR_MIX [B, N] (`what`: _lib.SVB_*)"""
        L.check(L.load().dust_svmpc_batch_set(self._h, int(what), _p(_f(value, self._shapes[int(what)]))))

    def get(self, what):
        """any of _lib.SVB_*: a settable quantity, or a record of the last iteration / forward"""
        out = np.empty(self._shapes[int(what)], np.float32)
        L.check(L.load().dust_svmpc_batch_get(self._h, int(what), _p(out)))
        return out

    HYPER_FIELDS = ("lr", "alpha", "temperature", "sigma_a", "chol_a", "sigma_p", "weighted_prior")

    def set_hyper(self, rows):
        """Per-environment hyper-parameters (dust_svmpc_batch_set_hyper): `rows` is a dict with every key of HYPER_FIELDS - lr, alpha,
        temperature and weighted_prior [B], the three sigmas [B], [B, 1] or [B, da] (diagonal) - or None: back to the prototype's values.
        While rows are set, optimize / forward / tick / episode run environment b under row b; the library refuses invalid rows."""
        if rows is None:
            L.check(L.load().dust_svmpc_batch_set_hyper(self._h, None))
            return
        B = self.B
        if sorted(rows) != sorted(self.HYPER_FIELDS):
            raise ValueError("rows has the keys %s, a row has %s" % (sorted(rows), sorted(self.HYPER_FIELDS)))
        cols = {}
        for k in self.HYPER_FIELDS:
            v = np.asarray(rows[k], np.float64 if k == "lr" else (np.int64 if k == "weighted_prior" else np.float32))
            if k in ("sigma_a", "chol_a", "sigma_p"):
                v = v.reshape(B, -1) if v.size in (B, B * self.da) else v
                if v.shape not in ((B, 1), (B, self.da)):
                    raise ValueError("%s has shape %s for %d environments with dim_a = %d" % (k, v.shape, B, self.da))
                v = np.broadcast_to(v, (B, self.da))
                v = np.concatenate([v, v[:, :1]], 1) if self.da == 1 else v  # (dim_a = 1: entry 1 repeats entry 0, nothing reads it)
            elif v.shape != (B,):
                raise ValueError("%s has shape %s for %d environments" % (k, v.shape, B))
            cols[k] = v
        arr = (L.SvmpcHyper * B)()
        for b in range(B):
            r = arr[b]
            r.lr, r.alpha, r.temperature = float(cols["lr"][b]), float(cols["alpha"][b]), float(cols["temperature"][b])
            r.weighted_prior = int(cols["weighted_prior"][b])
            for k in ("sigma_a", "chol_a", "sigma_p"):
                getattr(r, k)[:] = [float(cols[k][b, 0]), float(cols[k][b, 1])]
        L.check(L.load().dust_svmpc_batch_set_hyper(self._h, arr))

    def get_hyper(self):
        """The rows in force as a dict of arrays (dust_svmpc_batch_get_hyper): lr [B] float64, alpha / temperature [B], sigma_a / chol_a /
        sigma_p [B, da], weighted_prior [B] int32; the prototype's values where no rows are set."""
        B = self.B
        arr = (L.SvmpcHyper * B)()
        L.check(L.load().dust_svmpc_batch_get_hyper(self._h, arr))
        out = {"lr": np.array([r.lr for r in arr], np.float64), "alpha": np.array([r.alpha for r in arr], np.float32),
               "temperature": np.array([r.temperature for r in arr], np.float32),
               "weighted_prior": np.array([r.weighted_prior for r in arr], np.int32)}
        for k in ("sigma_a", "chol_a", "sigma_p"):
            out[k] = np.array([list(getattr(r, k))[:self.da] for r in arr], np.float32).reshape(B, self.da)
        return out

    def set_history(self, theta=False, filter=False):
        """What simulate() / dual_simulate() record from now on (dust_svmpc_batch_set_history): the particles after every period
        (`theta`) and, in dual_simulate(), the filters' particles every period's tick drew from (`filter`) - written by the episodes' own
        kernels, no launch added.  Both False: recording off, the buffers released.  Nothing else of the batch changes."""
        L.check(L.load().dust_svmpc_batch_set_history(self._h, (L.HIST_THETA if theta else 0) | (L.HIST_FILTER if filter else 0)))

    def history(self, which):
        """The last recording of one kind (dust_svmpc_batch_get_history) as a NaN-filled array: which = _lib.HIST_THETA -> [T, B, N, H, da];
        _lib.HIST_FILTER -> [T, B, Mp, P] (Mp, P: the filters of the dual_simulate() that recorded).  Rows (t, b) the recording call did
        not run are NaN, as the reference's frame has them.  The library answers DUST_ERR_STATE while nothing of that kind is recorded."""
        T = C.c_int(0)
        L.check(L.load().dust_svmpc_batch_get_history(self._h, int(which), C.byref(T), None))
        row = (self.N, self.H, self.da) if int(which) == L.HIST_THETA else self._hist_x_row
        out = np.full((T.value, self.B) + row, np.nan, np.float32)
        L.check(L.load().dust_svmpc_batch_get_history(self._h, int(which), None, _p(out)))
        return out

    def _inputs(self, states, n_steps, eps, params, eps_dev_ptr, keep_actions):
        B = self.B
        st = None if states is None else _f(states, (B, self.ds))  # (None: the library refuses)
        fl = L.SVMPC_BATCH_KEEP_ACTIONS if keep_actions else 0
        if eps_dev_ptr:
            e, fl = L.VP(eps_dev_ptr), fl | L.PTR_DEVICE
        else:
            e = None if eps is None else _f(eps, (B, n_steps, self.S, self.N, self.H, self.da))  # (the array: it stays alive through the call)
        pr = None
        if params is not None:
            pr = _f(params)
            want = (B, n_steps, self.M, max(self.P, 1))
            if pr.shape != want:
                raise ValueError("params has shape %s, the call reads %s" % (pr.shape, want))
        return st, e, pr, fl

    def optimize(self, states, n_steps, eps=None, params=None, active=None, eps_dev_ptr=None, keep_actions=False):
        """n_steps SVGD iterations of every active environment in one launch (dust_svmpc_batch_optimize).  states [B, ds]; eps
        [B, n_steps, S, N, H, da] or None (drawn on the device); params [B, n_steps, M, P] or None (no uncertain parameters)."""
        st, e, pr, fl = self._inputs(states, n_steps, eps, params, eps_dev_ptr, keep_actions)
        m, mp = _mask(active, self.B)
        L.check(L.load().dust_svmpc_batch_optimize(self._h, _p(st), int(n_steps), e if eps_dev_ptr else _vp(e), _p(pr), fl, mp))

    def forward(self, active=None, want_outputs=True):
        """SVMPC.forward of every active environment in one launch -> (a_seq [B, H, da], p_weights [B, N]); the rows of inactive
        environments are NaN.  want_outputs=False reads nothing back: the call does not wait for the device."""
        m, mp = _mask(active, self.B)
        a_seq = pw = None
        if want_outputs:
            a_seq, pw = np.full((self.B, self.H, self.da), np.nan, np.float32), np.full((self.B, self.N), np.nan, np.float32)
        L.check(L.load().dust_svmpc_batch_forward(self._h, mp, _p(a_seq), _p(pw)))
        return a_seq, pw

    def tick(self, states, n_steps, eps=None, params=None, active=None, eps_dev_ptr=None, keep_actions=False, want_outputs=True):
        """optimize + forward in ONE launch (dust_svmpc_batch_tick) -> (a_seq, p_weights) as forward()."""
        st, e, pr, fl = self._inputs(states, n_steps, eps, params, eps_dev_ptr, keep_actions)
        m, mp = _mask(active, self.B)
        a_seq = pw = None
        if want_outputs:
            a_seq, pw = np.full((self.B, self.H, self.da), np.nan, np.float32), np.full((self.B, self.N), np.nan, np.float32)
        L.check(L.load().dust_svmpc_batch_tick(self._h, _p(st), int(n_steps), e if eps_dev_ptr else _vp(e), _p(pr), fl, mp, _p(a_seq), _p(pw)))
        return a_seq, pw

    def episode(self, states, n_periods, n_steps, params=None, plant_params=None, active=None, want_pw=True, flags=0):
        """n_periods closed-loop periods of every active environment in ONE launch (dust_svmpc_batch_episode): per period the tick (noise
        drawn on the device), the plant's step with the first action of the chosen sequence under the environment's true parameters,
        the new state into the next tick.  states [B, ds]; params [T, B, n_steps, M, P] or None (no uncertain parameters);
        plant_params [B, P] or None (nominal plants).  -> (states [T, B, ds] after every step, actions [T, B, da], p_weights [T, B, N]
        or None, a_seq [B, H, da] of the last period); the rows of inactive environments are NaN.  flags: none is defined (the library
        refuses any)."""
        B, T = self.B, int(n_periods)
        st = None if states is None else _f(states, (B, self.ds))  # (None: the library refuses)
        pr = None
        if params is not None:
            pr = _f(params)
            want = (T, B, int(n_steps), self.M, max(self.P, 1))
            if pr.shape != want:
                raise ValueError("params has shape %s, the call reads %s" % (pr.shape, want))
        pl = _plant_rows(plant_params, B, self.P)
        _, mp = _mask(active, B)
        rows = max(T, 0)  # (n_periods < 1: the library refuses before it writes anything)
        xs, acts, a_seq = (np.full(sh, np.nan, np.float32) for sh in ((rows, B, self.ds), (rows, B, self.da), (B, self.H, self.da)))
        pw = np.full((rows, B, self.N), np.nan, np.float32) if want_pw else None
        L.check(L.load().dust_svmpc_batch_episode(self._h, _p(st), T, int(n_steps), _p(pr), _p(pl), int(flags), mp, _p(xs), _p(acts), _p(pw), _p(a_seq)))
        return xs, acts, pw, a_seq

    def simulate(self, states, n_periods, n_steps, params=None, plant_params=None, t0=0, warm_up=0, goal=None, goal_radius=None,
                 stop_on_crash=False, loss=None, status=None, active=None, want_pw=True, flags=0):
        """episode() under the reference's episode rules, still ONE launch (dust_svmpc_batch_simulate).  Period t is period t0 + t of the
        episode: below warm_up it is optimize alone and the plant gets a zero action; the family's instantaneous cost of every new state
        goes to `costs` and, as an fp32 running sum, to `loss`; with stop_on_crash a new position on an occupied cell ends the
        environment with loss = inf, status 2; with goal [ds] and goal_radius > 0, |goal - x|^2 <= radius^2 ends it with status 1.
        loss / status [B]: where a previous call left them (None: 0).  -> (states [T, B, ds], actions [T, B, da], p_weights [T, B, N] or
        None, costs [T, B], loss [B], status [B] int32, n_run [B] int32, a_seq [B, H, da]); rows the call did not write - past n_run[b],
        warm-up rows of p_weights, inactive environments - are NaN (n_run: -1)."""
        B, T = self.B, int(n_periods)
        st = None if states is None else _f(states, (B, self.ds))  # (None: the library refuses)
        pr = None
        if params is not None:
            pr = _f(params)
            want = (T, B, int(n_steps), self.M, max(self.P, 1))
            if pr.shape != want:
                raise ValueError("params has shape %s, the call reads %s" % (pr.shape, want))
        pl = _plant_rows(plant_params, B, self.P)
        ru = _episode_rules(self.ds, t0, warm_up, goal, goal_radius, stop_on_crash)
        _, mp = _mask(active, B)
        rows = max(T, 0)  # (n_periods < 1: the library refuses before it writes anything)
        xs, acts, costs, a_seq = (np.full(sh, np.nan, np.float32) for sh in ((rows, B, self.ds), (rows, B, self.da), (rows, B), (B, self.H, self.da)))
        pw = np.full((rows, B, self.N), np.nan, np.float32) if want_pw else None
        loss, status, n_run, IP = _rules_state(B, loss, status)
        L.check(L.load().dust_svmpc_batch_simulate(self._h, _p(st), T, int(n_steps), _p(pr), _p(pl), C.byref(ru), int(flags), mp, _p(xs), _p(acts),
                                                   _p(pw), _p(costs), _p(loss), status.ctypes.data_as(IP), n_run.ctypes.data_as(IP), _p(a_seq)))
        return xs, acts, pw, costs, loss, status, n_run, a_seq

    def dual_tick(self, mpf, states, actions_prev=None, n_steps=1, eps=None, mpf_steps=20, mpf_bw=None, seeds=None, active=None,
                  want_outputs=True, want_params=False, flags=0, eps_dev_ptr=None, keep_actions=False):
        """One control period of the DuSt-MPC loop for every active environment in one C call (dust_svmpc_dual_batch_tick): the filters'
        update for (actions_prev[b], states[b]) - skipped when actions_prev is None -, then ONE launch of n_steps SVGD iterations, whose
        dynamics samples are drawn inside the kernel from every environment's refreshed prior, and forward().  mpf: an `MpfBatch` of B
        environments; seeds [B]: the Philox key of every environment's draws; eps as tick().  -> (a_seq [B, H, da] before the roll,
        p_weights [B, N], params [B, n_steps, M, P] or None, bw_used [B]); the rows of inactive environments are NaN.
        want_outputs=False reads nothing back: the call does not wait for the device."""
        B = self.B
        st, e, _, fl = self._inputs(states, n_steps, eps, None, eps_dev_ptr, keep_actions)
        ap = None if actions_prev is None else _f(actions_prev, (B, self.da))
        sd, sp = _seeds(seeds, B)
        _, mp = _mask(active, B)
        a_seq = pw = bw = None
        if want_outputs:
            a_seq, pw, bw = (np.full(sh, np.nan, np.float32) for sh in ((B, self.H, self.da), (B, self.N), (B,)))
        pout = np.full((B, int(n_steps), self.M, max(self.P, 1)), np.nan, np.float32) if want_params else None
        L.check(L.load().dust_svmpc_dual_batch_tick(self._h, mpf._h, _p(st), _p(ap), int(n_steps), e if eps_dev_ptr else _vp(e), int(flags) | fl,
                                                    int(mpf_steps), float(-1.0 if mpf_bw is None else mpf_bw), sp, mp,
                                                    _p(a_seq), _p(pw), _p(pout), _p(bw)))
        return a_seq, pw, pout, bw

    def dual_episode(self, mpf, states, n_periods, n_steps, actions_prev=None, mpf_steps=20, mpf_bw=None, seeds=None, plant_params=None,
                     active=None, want_pw=True):
        """n_periods control periods of the DuSt-MPC loop for every active environment in one C call (dust_svmpc_dual_batch_episode): per
        period the filters' update for (a_{t-1}, x_t) - period 0: actions_prev, skipped when it is None -, the tick of dual_tick() with
        the noise drawn on the device, the plant's step with the first action of the chosen sequence under the environment's true
        parameters; no host round trip between periods.  states [B, ds]; seeds [T, B]: period t's Philox keys; plant_params [B, P] or
        None (nominal plants).  -> (states [T, B, ds] after every step, actions [T, B, da], p_weights [T, B, N] or None, bw [T, B],
        a_seq [B, H, da] of the last period); the rows of inactive environments are NaN.  The pair (actions[-1], states[-1]) is still
        to be folded into the filters: hand it to the next call."""
        B, T = self.B, int(n_periods)
        st = None if states is None else _f(states, (B, self.ds))  # (None: the library refuses)
        ap = None if actions_prev is None else _f(actions_prev, (B, self.da))
        rows = max(T, 0)  # (n_periods < 1: the library refuses before it reads or writes anything)
        sd, sp = _period_seeds(seeds, rows, B)
        pl = _plant_rows(plant_params, B, self.P)
        _, mp = _mask(active, B)
        xs, acts, bw, a_seq = (np.full(sh, np.nan, np.float32) for sh in ((rows, B, self.ds), (rows, B, self.da), (rows, B), (B, self.H, self.da)))
        pw = np.full((rows, B, self.N), np.nan, np.float32) if want_pw else None
        L.check(L.load().dust_svmpc_dual_batch_episode(self._h, mpf._h, _p(st), _p(ap), T, int(n_steps), int(mpf_steps),
                                                       float(-1.0 if mpf_bw is None else mpf_bw), sp, _p(pl), 0, mp,
                                                       _p(xs), _p(acts), _p(pw), _p(bw), _p(a_seq)))
        return xs, acts, pw, bw, a_seq

    def dual_optimize(self, mpf, states, actions_prev=None, n_steps=1, eps=None, mpf_steps=20, mpf_bw=None, seeds=None, active=None,
                      want_outputs=True, want_params=False, flags=0, eps_dev_ptr=None, keep_actions=False):
        """One WARM-UP period of the DuSt-MPC loop for every active environment in one C call (dust_svmpc_dual_batch_optimize): dual_tick()
        without forward() - the filters' update, then the n_steps SVGD iterations under rows drawn from the refreshed priors; no roll,
        no sequence, no weights.  -> (params [B, n_steps, M, P] or None, bw_used [B] or None); the rows of inactive environments are NaN."""
        B = self.B
        st, e, _, fl = self._inputs(states, n_steps, eps, None, eps_dev_ptr, keep_actions)
        ap = None if actions_prev is None else _f(actions_prev, (B, self.da))
        sd, sp = _seeds(seeds, B)
        _, mp = _mask(active, B)
        bw = np.full((B,), np.nan, np.float32) if want_outputs else None
        pout = np.full((B, int(n_steps), self.M, max(self.P, 1)), np.nan, np.float32) if want_params else None
        L.check(L.load().dust_svmpc_dual_batch_optimize(self._h, mpf._h, _p(st), _p(ap), int(n_steps), e if eps_dev_ptr else _vp(e), int(flags) | fl,
                                                        int(mpf_steps), float(-1.0 if mpf_bw is None else mpf_bw), sp, mp, _p(pout), _p(bw)))
        return pout, bw

    def dual_simulate(self, mpf, states, n_periods, n_steps, actions_prev=None, mpf_steps=20, mpf_bw=None, seeds=None, plant_params=None,
                      t0=0, warm_up=0, goal=None, goal_radius=None, stop_on_crash=False, loss=None, status=None, active=None, want_pw=True,
                      flags=0):
        """dual_episode() under the reference's episode rules, in one C call (dust_svmpc_dual_batch_simulate): period t is period t0 + t of
        the episode; below warm_up the tick runs without forward() and the plant gets a zero action while the filters keep updating; the
        cost of every new state goes to `costs` and, as an fp32 running sum, to `loss`; crash (status 2, loss inf) and goal (status 1)
        stop an environment on both sides - no further filter update, no tick.  loss / status [B]: where a previous call left them.
        -> (states [T, B, ds], actions [T, B, da], p_weights [T, B, N] or None, bw [T, B], costs [T, B], loss [B], status [B] int32,
        n_run [B] int32, a_seq [B, H, da]); rows the call did not write - past n_run[b], warm-up rows of p_weights, inactive
        environments - are NaN (n_run: -1)."""
        B, T = self.B, int(n_periods)
        st = None if states is None else _f(states, (B, self.ds))  # (None: the library refuses)
        ap = None if actions_prev is None else _f(actions_prev, (B, self.da))
        rows = max(T, 0)  # (n_periods < 1: the library refuses before it reads or writes anything)
        sd, sp = _period_seeds(seeds, rows, B)
        pl = _plant_rows(plant_params, B, self.P)
        ru = _episode_rules(self.ds, t0, warm_up, goal, goal_radius, stop_on_crash)
        _, mp = _mask(active, B)
        xs, acts, bw, costs, a_seq = (np.full(sh, np.nan, np.float32)
                                      for sh in ((rows, B, self.ds), (rows, B, self.da), (rows, B), (rows, B), (B, self.H, self.da)))
        pw = np.full((rows, B, self.N), np.nan, np.float32) if want_pw else None
        loss, status, n_run, IP = _rules_state(B, loss, status)
        L.check(L.load().dust_svmpc_dual_batch_simulate(self._h, mpf._h, _p(st), _p(ap), T, int(n_steps), int(mpf_steps),
                                                        float(-1.0 if mpf_bw is None else mpf_bw), sp, _p(pl), C.byref(ru), int(flags), mp,
                                                        _p(xs), _p(acts), _p(pw), _p(bw), _p(costs), _p(loss), status.ctypes.data_as(IP),
                                                        n_run.ctypes.data_as(IP), _p(a_seq)))
        self._hist_x_row = (int(mpf.Mp), int(mpf.P))
        return xs, acts, pw, bw, costs, loss, status, n_run, a_seq


_STEP_IDS = {"argmax": L.STEP_ARGMAX, "average": L.STEP_AVERAGE, "external": L.STEP_EXTERNAL}


class DiscoBatch(_BatchHandle):
    """B independent MultiDISCO controllers in one launch (dust_disco_batch_*): per environment a state, a_mat, a_seq, a_mix, a noise
    stream and parameter rows; everything else is the prototype context's.  `ctx` is the batch's inner context (borrowed) for sync() and
    profile() / profile_get()."""

    _destroy, _clone = "dust_disco_batch_destroy", "dust_disco_batch_clone"

    def __init__(self, proto=None, n_envs=1, seeds=None, _handle=None):
        self._h = None
        lib = L.load()
        if _handle is None:
            sd, sp = _seeds(seeds, int(n_envs))
            h = L.VP()
            L.check(lib.dust_disco_batch_create(proto._h, int(n_envs), sp, C.byref(h)))
            _handle = h
        self._h = _handle
        self.B = int(n_envs)
        inner = L.VP()
        L.check(lib.dust_disco_batch_ctx(self._h, C.byref(inner)))
        self.ctx = Context(_handle=inner)
        self.ctx._borrowed = True
        c = self.ctx
        self.N, self.S, self.H, self.da, self.ds, self.P, self.M = c.N, c.S, c.H, c.da, c.ds, c.P, c.M
        B, N, S, H, da = self.B, self.N, self.S, self.H, self.da
        self._shapes = {L.DCB_A_MAT: (B, N, H, da), L.DCB_A_SEQ: (B, H, da), L.DCB_A_MIX: (B, N), L.DCB_COSTS: (B, S, N),
                        L.DCB_OMEGA: (B, S, N), L.DCB_ACTIONS: (B, S, N, H, da)}

    def set(self, what, value):
        """A_MAT [B, N, H, da], A_SEQ [B, H, da] (`what`: _lib.DCB_*)"""
        L.check(L.load().dust_disco_batch_set(self._h, int(what), _p(_f(value, self._shapes[int(what)]))))

    def get(self, what):
        """any of _lib.DCB_*: a settable quantity, a_mix, or a record of the last forward"""
        out = np.empty(self._shapes[int(what)], np.float32)
        L.check(L.load().dust_disco_batch_get(self._h, int(what), _p(out)))
        return out

    def _forward_inputs(self, states, actions, params, around_a_mat, keep_actions):
        B = self.B
        st = None if states is None else _f(states, (B, self.ds))  # (None: the library refuses)
        act = None if actions is None else _f(actions, (B, self.S, self.N, self.H, self.da))
        pr = None
        if params is not None:
            pr = _f(params)
            want = (B, self.M, max(self.P, 1))
            if pr.shape != want:
                raise ValueError("params has shape %s, the call reads %s" % (pr.shape, want))
        return st, act, pr, (L.EPS_AROUND_A_MAT if around_a_mat else 0) | (L.SVMPC_BATCH_KEEP_ACTIONS if keep_actions else 0)

    def _step_inputs(self, strategy, steps, ext_actions):
        sid = _STEP_IDS.get(strategy, -1) if isinstance(strategy, str) else int(strategy)
        ext = None if ext_actions is None else _f(ext_actions, (self.B, self.H, self.da))
        rows = min(max(int(steps), 0), self.H)  # (steps outside [1, H]: the library refuses before it writes anything)
        return sid, ext, np.full((self.B, rows, self.da), np.nan, np.float32)

    def forward(self, states, actions=None, params=None, active=None, around_a_mat=False, keep_actions=False, flags=0):
        """MultiDISCO.forward of every active environment in one launch (dust_disco_batch_forward).  states [B, ds]; actions
        [B, S, N, H, da] recorded, or None (drawn on the device); params [B, M, P] (the sigma points under sigma weights) or None (no
        uncertain parameters).  Nothing is read back: the call does not wait for the device."""
        st, act, pr, fl = self._forward_inputs(states, actions, params, around_a_mat, keep_actions)
        _, mp = _mask(active, self.B)
        L.check(L.load().dust_disco_batch_forward(self._h, _p(st), _p(act), _p(pr), fl | int(flags), mp))

    def step(self, strategy="argmax", steps=1, ext_actions=None, active=None):
        """MultiDISCO.step of every active environment in one launch -> next_actions [B, steps, da]; inactive rows are NaN."""
        sid, ext, nxt = self._step_inputs(strategy, steps, ext_actions)
        _, mp = _mask(active, self.B)
        L.check(L.load().dust_disco_batch_step(self._h, sid, int(steps), _p(ext), mp, _p(nxt)))
        return nxt

    def tick(self, states, strategy="argmax", steps=1, actions=None, params=None, ext_actions=None, active=None, around_a_mat=False,
             keep_actions=False, flags=0):
        """forward + step in ONE launch (dust_disco_batch_tick) -> next_actions as step()."""
        st, act, pr, fl = self._forward_inputs(states, actions, params, around_a_mat, keep_actions)
        sid, ext, nxt = self._step_inputs(strategy, steps, ext_actions)
        _, mp = _mask(active, self.B)
        L.check(L.load().dust_disco_batch_tick(self._h, _p(st), _p(act), _p(pr), fl | int(flags), mp, sid, int(steps), _p(ext), _p(nxt)))
        return nxt

    def episode(self, states, n_periods, strategy="average", params=None, plant_params=None, params_once=False, rules=None, loss=None,
                status=None, active=None, flags=0):
        """n_periods closed-loop periods of every active environment in ONE launch (dust_disco_batch_episode): per period forward (noise
        drawn on the device), step(strategy, 1), the plant's step under the environment's true parameters.  params [T, B, M, P], or
        [B, M, P] with params_once; plant_params [B, P] or None (nominal plants).  rules: None, or a dict with any of t0, goal [ds],
        goal_radius, stop_on_crash (and warm_up, which must be 0) - the reference's episode rules as SvmpcBatch.simulate applies them;
        loss / status [B]: where a previous call left them.  -> (states [T, B, ds], actions [T, B, da], a_seq [B, H, da]) without
        rules, (states, actions, costs [T, B], loss [B], status [B], n_run [B], a_seq) with them; rows the call did not write are NaN
        (n_run: -1)."""
        B, T = self.B, int(n_periods)
        st = None if states is None else _f(states, (B, self.ds))  # (None: the library refuses)
        pr = None
        if params is not None:
            pr = _f(params)
            want = (B, self.M, max(self.P, 1)) if params_once else (T, B, self.M, max(self.P, 1))
            if pr.shape != want:
                raise ValueError("params has shape %s, the call reads %s" % (pr.shape, want))
        pl = _plant_rows(plant_params, B, self.P)
        sid = _STEP_IDS.get(strategy, -1) if isinstance(strategy, str) else int(strategy)
        _, mp = _mask(active, B)
        rows = max(T, 0)  # (n_periods < 1: the library refuses before it writes anything)
        xs, acts, a_seq = (np.full(sh, np.nan, np.float32) for sh in ((rows, B, self.ds), (rows, B, self.da), (B, self.H, self.da)))
        fl = int(flags) | (L.DISCO_PARAMS_ONCE if params_once else 0)
        if rules is None:
            L.check(L.load().dust_disco_batch_episode(self._h, _p(st), T, _p(pr), _p(pl), sid, None, fl, mp, _p(xs), _p(acts), None, None,
                                                      None, None, _p(a_seq)))
            return xs, acts, a_seq
        unknown = set(rules) - {"t0", "warm_up", "goal", "goal_radius", "stop_on_crash"}
        if unknown:
            raise ValueError("rules has the unknown keys %s" % sorted(unknown))
        ru = _episode_rules(self.ds, rules.get("t0", 0), rules.get("warm_up", 0), rules.get("goal"), rules.get("goal_radius"),
                            rules.get("stop_on_crash", False))
        costs = np.full((rows, B), np.nan, np.float32)
        loss, status, n_run, IP = _rules_state(B, loss, status)
        L.check(L.load().dust_disco_batch_episode(self._h, _p(st), T, _p(pr), _p(pl), sid, C.byref(ru), fl, mp, _p(xs), _p(acts), _p(costs),
                                                  _p(loss), status.ctypes.data_as(IP), n_run.ctypes.data_as(IP), _p(a_seq)))
        return xs, acts, costs, loss, status, n_run, a_seq


class MpfBatch(_BatchHandle):
    """B dynamics filters of one configuration, updated in one launch (dust_mpf_batch_*): per environment its particles, optimiser
    state, observations, past action and bandwidths; model, obs_std, optimiser options, Mp and P are the prototype filter's.
    Environment b computes what a lone `MpfContext` created under DUST_MPF_GRID=0 computes on its inputs, bit for bit."""

    _destroy, _clone = "dust_mpf_batch_destroy", "dust_mpf_batch_clone"

    def __init__(self, proto=None, n_envs=1, _handle=None, _like=None):
        self._h = None
        like = proto if _like is None else _like
        self.Mp, self.P, self.ds, self.da = like.Mp, like.P, like.ds, like.da
        self.B = int(n_envs)
        if _handle is None:
            h = L.VP()
            L.check(L.load().dust_mpf_batch_create(proto._h, self.B, C.byref(h)))
            _handle = h
        self._h = _handle
        if isinstance(like, MpfBatch):  # (a clone: the source's prototype)
            self._proto_hyper = dict(like._proto_hyper)
        else:  # what a field left out of a row takes: the values of a batch without rows
            row = (L.MpfHyper * self.B)()
            L.check(L.load().dust_mpf_batch_get_hyper(self._h, row))
            self._proto_hyper = {k: getattr(row[0], k) for k in self.HYPER_FIELDS}

    def set_particles(self, x):
        L.check(L.load().dust_mpf_batch_set_particles(self._h, _p(_f(x, (self.B, self.Mp, self.P)))))

    def get_particles(self):
        out = np.empty((self.B, self.Mp, self.P), np.float32)
        L.check(L.load().dust_mpf_batch_get_particles(self._h, _p(out)))
        return out

    def set_obs(self, obs):
        """Every environment's observation [B, ds]: the state the next update's one-step prediction starts from."""
        L.check(L.load().dust_mpf_batch_set_obs(self._h, _p(_f(obs, (self.B, self.ds)))))

    def get_prior_bw(self):
        """[B, P] bandwidths of every environment's current prior."""
        out = np.empty((self.B, 4), np.float32)
        L.check(L.load().dust_mpf_batch_get_prior_bw(self._h, _p(out)))
        return out[:, :self.P].copy()

    def stats(self):
        """{'launches': kernel launches made for the filter side, 'calls': updates and dual ticks}."""
        n = (C.c_longlong * 2)()
        L.check(L.load().dust_mpf_batch_stats(self._h, n))
        return {"launches": int(n[0]), "calls": int(n[1])}

    HYPER_FIELDS = ("lr", "obs_std", "bw", "bw_scale")
    HYPER_DTYPE = np.dtype([("lr", np.float64), ("obs_std", np.float32), ("bw", np.float32), ("bw_scale", np.float32)])

    def set_hyper(self, rows):
        """Per-environment filter hyper-parameters (dust_mpf_batch_set_hyper): `rows` is a list of B dicts or a structured array [B]
        with any of lr, obs_std, bw, bw_scale - fields left out take the prototype's values (bw: 0, Silverman's rule) - or None: back to
        the prototype's.  While rows are set environment b updates under row b: its bandwidth is bw when that is > 0, else Silverman's
        rule on its particles times bw_scale, and the bw of optimize() / the mpf_bw of the dual calls must be None or <= 0.  Copies and
        deep copies carry the rows; the library refuses invalid rows and skid-steer / cart-pole batches."""
        if rows is None:
            L.check(L.load().dust_mpf_batch_set_hyper(self._h, None))
            return
        B = self.B
        if isinstance(rows, np.ndarray) and rows.dtype.names:
            unknown = set(rows.dtype.names) - set(self.HYPER_FIELDS)
            rows = [{k: r[k] for k in rows.dtype.names} for r in rows.reshape(-1)]
        else:
            rows = [dict(r) for r in rows]
            unknown = set().union(*[set(r) for r in rows]) - set(self.HYPER_FIELDS) if rows else set()
        if unknown:
            raise ValueError("a filter hyper-parameter row has the fields %s (got %s)" % (list(self.HYPER_FIELDS), sorted(unknown)))
        if len(rows) != B:
            raise ValueError("%d rows for %d environments" % (len(rows), B))
        arr = (L.MpfHyper * B)()
        for b, r in enumerate(rows):
            for k in self.HYPER_FIELDS:
                setattr(arr[b], k, float(r[k]) if k in r else self._proto_hyper[k])
        L.check(L.load().dust_mpf_batch_set_hyper(self._h, arr))

    @property
    def hyper(self):
        """The rows in force as a structured array [B] (HYPER_DTYPE; dust_mpf_batch_get_hyper): the prototype's values, with bw = 0,
        where none are set."""
        arr = (L.MpfHyper * self.B)()
        L.check(L.load().dust_mpf_batch_get_hyper(self._h, arr))
        out = np.zeros(self.B, self.HYPER_DTYPE)
        for b, r in enumerate(arr):
            out[b] = (r.lr, r.obs_std, r.bw, r.bw_scale)
        return out

    def optimize(self, actions, new_obs, bw, n_steps, active=None):
        """B x MpfContext.optimize in one launch (dust_mpf_batch_optimize).  actions [B, da], new_obs [B, ds]; bw None or <= 0:
        Silverman's rule per environment on the device (with rows set: row b's bandwidth).  -> (grad_norms [B, n_steps], bw_used [B]);
        NaN rows for inactive environments."""
        a = None if actions is None else _f(actions, (self.B, self.da))
        o = None if new_obs is None else _f(new_obs, (self.B, self.ds))
        _, mp = _mask(active, self.B)
        gn = np.full((self.B, max(int(n_steps), 1)), np.nan, np.float32)
        bwu = np.full(self.B, np.nan, np.float32)
        L.check(L.load().dust_mpf_batch_optimize(self._h, _p(a), _p(o), float(-1.0 if bw is None else bw), int(n_steps), mp, _p(bwu),
                                                 _p(gn) if n_steps > 0 else None))
        return gn[:, :n_steps], bwu


class MpfContext:
    def __init__(self, init_particles, initial_obs, model="pendulum", uncertain_params=("length", "mass"), log_space=False,
                 obs_std=0.1, lr=1e-3, bw_scale=1.0, init_bw=0.1, device=0, grid=None, _handle=None, optimizer="SGD", betas=(0.9, 0.999),
                 eps=1e-8, optim=None, **model_kw):
        lib = L.load()
        x = _f(init_particles)
        self.Mp, self.P = x.shape
        if _handle is not None:
            self._h = _handle
            return
        c = L.MpfConfig()
        c.abi_version, c.device, c.n_particles, c.dim_p = L.ABI_VERSION, device, self.Mp, self.P
        c.model_cfg = make_config(model=model, uncertain_params=uncertain_params, params_log_space=log_space, device=device, **model_kw)
        c.dim_s, c.dim_a, c.model = c.model_cfg.dim_s, c.model_cfg.dim_a, c.model_cfg.model
        c.log_space, c.obs_std, c.lr, c.bw_scale, c.init_bw = int(log_space), obs_std, lr, bw_scale, init_bw
        self.ds, self.da = c.dim_s, c.dim_a
        h = L.VP()
        L.check(lib.dust_mpf_create(C.byref(c), _p(x), _p(_f(initial_obs, (c.dim_s,))), C.byref(h)))
        self._h = h
        if c.model == L.MODEL_SKID_STEER:
            self.set_skid_steer(uncertain_params=uncertain_params, min_a=c.model_cfg.min_a, max_a=c.model_cfg.max_a,
                                **{k: model_kw[k] for k in ("x_icr", "wheel_radius", "axial_distance") if k in model_kw})
        if c.model == L.MODEL_CARTPOLE:
            self.set_cartpole(uncertain_params=uncertain_params, **{k: model_kw[k] for k in CARTPOLE_PARAMS if k in model_kw})
        if grid is not None:
            g = _f(grid)
            L.check(lib.dust_mpf_set_grid(self._h, _p(g), g.shape[0], g.shape[1], float(int(g.shape[0] / 2)), float(int(g.shape[1] / 2))))
        from . import optim as _optim

        if optim is not None and not _optim.is_plain(optim):  # dust_amd.optim.optimizer_config(...): its state persists as Adam's does
            L.check(lib.dust_mpf_set_optimizer_ex(self._h, C.byref(_optim.to_struct(optim))))
            return
        if optimizer not in ("SGD", "Adam"):
            raise NotImplementedError("MPF optimiser %r: the device filter implements SGD and Adam" % (optimizer,))
        if optimizer == "Adam":  # the reference's class default (svgd.py:115); its state persists across optimize() calls
            L.check(lib.dust_mpf_set_optimizer(self._h, L.OPT_ADAM, float(betas[0]), float(betas[1]), float(eps)))

    def close(self):
        if getattr(self, "_h", None) is not None:
            L.load().dust_mpf_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_skid_steer(self, x_icr=0.2, wheel_radius=0.0625, axial_distance=0.475, min_a=(-0.5, -0.5), max_a=(0.5, 0.5), uncertain_params=()):
        """The filter's SkidSteerRobot (dust_mpf_set_skid_steer): `uncertain_params` name the particle columns, in order; the other
        parameters stay at the given values; min_a / max_a are the wheel-speed bounds."""
        up = list(uncertain_params or ())
        g = L.SkidConfig()

        def par(name, value):
            return L.Param(L.PARAM_SAMPLED, up.index(name), float(value)) if name in up else L.Param(L.PARAM_PYFLOAT, 0, float(value))

        g.x_icr, g.wheel_radius, g.axial_distance = par("x_icr", x_icr), par("wheel_radius", wheel_radius), par("axial_distance", axial_distance)
        for d in range(2):
            g.min_wheel_speed[d], g.max_wheel_speed[d] = float(min_a[d]), float(max_a[d])
        L.check(L.load().dust_mpf_set_skid_steer(self._h, C.byref(g)))

    def set_cartpole(self, g=9.8, f_mag=10.0, mass_cart=1.0, mass_pole=0.1, length=1.0, mu_c=0.5e-3, mu_p=2e-6, uncertain_params=()):
        """The filter's CartPoleModel (dust_mpf_set_cartpole): `uncertain_params` name the particle columns, in order; the other
        parameters stay at the given values."""
        cfg = _cartpole_struct(dict(g=g, f_mag=f_mag, mass_cart=mass_cart, mass_pole=mass_pole, length=length, mu_c=mu_c, mu_p=mu_p),
                               list(uncertain_params or ()))
        L.check(L.load().dust_mpf_set_cartpole(self._h, C.byref(cfg)))

    def silverman(self):
        """silvermans_rule of the pooled particles times bw_scale, on the device (dust_mpf_silverman)."""
        bw = C.c_float(0.0)
        L.check(L.load().dust_mpf_silverman(self._h, C.cast(C.byref(bw), L.FP)))
        return float(bw.value)

    def clone(self):
        h = L.VP()
        L.check(L.load().dust_mpf_clone(self._h, C.byref(h)))
        m = MpfContext.__new__(MpfContext)
        m._h, m.Mp, m.P, m.ds, m.da = h, self.Mp, self.P, self.ds, self.da
        return m

    def __deepcopy__(self, memo):
        return self.clone()

    def batch(self, n_envs):
        """`n_envs` copies of this filter - particles, observations, optimiser state, bandwidths - updated in one launch
        (dust_mpf_batch_create): the batch keeps its own copy of the filter."""
        return MpfBatch(self, n_envs)

    def condition(self, action, new_obs):
        a = None if action is None else _f(action).reshape(-1)
        L.check(L.load().dust_mpf_condition(self._h, _p(a), _p(_f(new_obs, (self.ds,)))))

    def set_ctrl_noise(self, z):
        """Recorded control-noise draws [n][da] for the next phi / optimize steps (one per SVGD step; likelihoods.py:30-46 ->
        particle.py:145-148); None: the library's own generator."""
        if z is None:
            L.check(L.load().dust_mpf_set_ctrl_noise(self._h, None, 0))
            return
        z = _f(z, (-1, self.da))
        L.check(L.load().dust_mpf_set_ctrl_noise(self._h, _p(z), int(z.shape[0])))

    def phi(self, bw):
        out = np.empty((self.Mp, self.P), np.float32)
        L.check(L.load().dust_mpf_phi(self._h, float(bw), _p(out)))
        return out

    def optimize(self, action, new_obs, bw, n_steps):
        a = None if action is None else _f(action).reshape(-1)
        o = None if new_obs is None else _f(new_obs, (self.ds,))
        gn = np.empty(max(n_steps, 1), np.float32)
        L.check(L.load().dust_mpf_optimize(self._h, _p(a), _p(o), float(bw), n_steps, _p(gn)))
        return gn[:n_steps]

    def get_particles(self):
        out = np.empty((self.Mp, self.P), np.float32)
        L.check(L.load().dust_mpf_get_particles(self._h, _p(out)))
        return out

    def set_particles(self, x):
        L.check(L.load().dust_mpf_set_particles(self._h, _p(_f(x, (self.Mp, self.P)))))

    def get_prior(self):
        means = np.empty((self.Mp, self.P), np.float32)
        bw = C.c_float(0)
        L.check(L.load().dust_mpf_get_prior(self._h, _p(means), C.cast(C.byref(bw), L.FP)))
        return means, bw.value

    def set_prior_bw(self, bw):
        """Per-dimension bandwidths of the current prior (MPF(bw=None): bw_silverman of the particle columns, mpf.py:31-36)."""
        b = np.ascontiguousarray(np.asarray(bw, np.float32).reshape(-1))
        L.check(L.load().dust_mpf_set_prior_bw(self._h, _p(b), int(b.size)))

    def get_prior_bw(self):
        out = np.empty(self.P, np.float32)
        L.check(L.load().dust_mpf_get_prior_bw(self._h, _p(out)))
        return out

    def stats(self):
        """{'grid': optimize() calls served by the multi-workgroup kernel, 'fallback': those re-run by the single-workgroup one}."""
        import ctypes as C
        n = (C.c_longlong * 2)()
        L.check(L.load().dust_mpf_stats(self._h, n))
        return {"grid": int(n[0]), "fallback": int(n[1])}

    def prior_sample(self, n, seed=0):
        out = np.empty((n, self.P), np.float32)
        L.check(L.load().dust_mpf_prior_sample(self._h, n, seed, _p(out)))
        return out

    def sigma_points(self, scale):
        """[2P + 1, P] sigma points of the prior's mean and diagonal variance for a Merwe transform with lambda + n = scale."""
        out = np.empty((2 * self.P + 1, self.P), np.float32)
        L.check(L.load().dust_mpf_sigma_points(self._h, float(scale), _p(out)))
        return out

    def prior_log_prob(self, x):
        x = _f(x, (-1, self.P))
        out = np.empty(x.shape[0], np.float32)
        L.check(L.load().dust_mpf_prior_log_prob(self._h, x.shape[0], _p(x), _p(out)))
        return out
