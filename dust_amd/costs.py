"""Cost-function families the HIP kernels implement, and recognition of user callables.

The reference takes arbitrary Python callables (`inst_cost_fn`, `term_cost_fn`; the pendulum ones live in the demo script,
demo/pendulum_example.py:21-28).  A GPU kernel cannot call back into Python and this backend has no CPU fallback, so a
callable is accepted only if it belongs to a known family: either it is one of the tagged callables below / a bound
`Particle.default_*_cost`, or - so that the demo's own `inst_cost` works unchanged - it is PROBED on a few states and
matches  w_cos (cos th - 1)^2 + w_vel thd^2  to 1e-6.  Anything else raises NotImplementedError."""
import torch


class PendulumQuadCos:
    """inst = w_cos (cos th - 1)^2 + w_vel thd^2 ; term = inst (demo/pendulum_example.py:21-28)."""

    family = "pendulum_quadcos"

    def __init__(self, w_cos=50.0, w_vel=1.0):
        self.w_cos, self.w_vel = float(w_cos), float(w_vel)

    def inst_cost(self, states, controls=None, n_pol=1, debug=None):
        th, thd = states.chunk(2, dim=1)
        return self.w_cos * (th.cos() - 1) ** 2 + self.w_vel * thd ** 2

    def term_cost(self, states, n_pol=1, debug=None):
        return self.inst_cost(states).squeeze()


class QuadraticCost:
    """Quadratic state / control cost for any model (the skid-steer and cart-pole families use it: the reference ships no cost for these models and
    its MultiDISCO takes any callable with this signature, disco.py:294-346):
        inst(x, a) = sum_k w_state[k] (x_k - goal_k)^2 + sum_d w_ctrl[d] a_d^2        term(x) = sum_k w_term[k] (x_k - goal_k)^2
    `inst_cost` / `term_cost` are plain torch, so the same object drives the reference's controller and this one's kernels."""

    family = "quadratic"

    def __init__(self, goal, w_state, w_term=None, w_ctrl=None):
        self.goal = torch.as_tensor(goal, dtype=torch.float).reshape(-1)
        self.w_state = torch.as_tensor(w_state, dtype=torch.float).reshape(-1)
        self.w_term = self.w_state.clone() if w_term is None else torch.as_tensor(w_term, dtype=torch.float).reshape(-1)
        self.w_ctrl = None if w_ctrl is None else torch.as_tensor(w_ctrl, dtype=torch.float).reshape(-1)

    def inst_cost(self, states, controls=None, n_pol=1, debug=None):
        c = (((states - self.goal) ** 2) * self.w_state).sum(-1)
        if controls is not None and self.w_ctrl is not None:
            c = c + ((controls ** 2) * self.w_ctrl).sum(-1)
        return c

    def term_cost(self, states, n_pol=1, debug=None):
        return (((states - self.goal) ** 2) * self.w_term).sum(-1)


class NavigationCost(QuadraticCost):
    """The quadratic family plus the obstacle term of Particle.default_inst_cost / default_term_cost (particle.py:170-225) on the position
    plane states[..., 0:2] - the skid-steer family's navigation cost:
        inst(x, a) = quad(x) + ctrl(a) + w_obs * obst_map.get_collisions(x[..., 0:2])        term(x) = quad(x) + w_obs * get_collisions(...)
    `obst_map` is anything with get_collisions, .map and .cell_size (obstacle_map.py:64-93): this package's ObstacleMap or the reference's.
    Plain torch like QuadraticCost, so the same object drives the reference's controllers."""

    family = "navigation"

    def __init__(self, goal, w_state, w_term=None, w_ctrl=None, obst_map=None, w_obs=0.0):
        super().__init__(goal, w_state, w_term, w_ctrl)
        self.obst_map, self.w_obs = obst_map, float(w_obs)

    def _obst(self, states):
        if self.obst_map is None:
            if self.w_obs != 0.0:
                raise ValueError("NavigationCost(w_obs != 0) needs an obst_map (particle.py:172-175 reads self.obst_map)")
            return 0.0
        if getattr(self.obst_map, "map_torch", None) is None:
            self.obst_map.convert_map()
        return self.w_obs * self.obst_map.get_collisions(states[..., 0:2])

    def inst_cost(self, states, controls=None, n_pol=1, debug=None):
        return QuadraticCost.inst_cost(self, states, controls) + self._obst(states)  # particle.py:197: state + control + obstacle

    def term_cost(self, states, n_pol=1, debug=None):
        return QuadraticCost.term_cost(self, states) + self._obst(states)  # particle.py:225

    def grid(self):
        """The occupancy grid as the fp32 array Context(grid=) takes, or None without a map."""
        import numpy as np

        return None if self.obst_map is None else np.ascontiguousarray(np.asarray(self.obst_map.map, dtype=np.float32))

    def grid_key(self):
        """(shape, SHA-1 of the fp32 map) for a controller's context key, or None without a map.  The controllers ask on every tick, so
        the digest is kept and taken again only when the map is another one: obst_map.map reassigned (another array object; the last one
        is held, so its id cannot return), another shape, or - an edit in place - other row or column sums."""
        import hashlib

        import numpy as np

        if self.obst_map is None:
            return None
        m = np.asarray(self.obst_map.map)
        cols, rows = m.sum(axis=0, dtype=np.float64), m.sum(axis=1, dtype=np.float64)
        stamp = (m.shape, str(m.dtype), float(cols @ np.arange(1.0, cols.size + 1.0)), float(rows @ np.arange(1.0, rows.size + 1.0)))
        kept = getattr(self, "_grid_key", None)
        if kept is None or kept[0] is not self.obst_map.map or kept[1] != stamp:
            kept = self._grid_key = (self.obst_map.map, stamp, (m.shape, hashlib.sha1(self.grid().tobytes()).hexdigest()))
        return kept[2]


def cost_grid(inst_cost_fn):
    """The map a cost object carries (NavigationCost: the skid-steer model has none of its own), or None."""
    owner = getattr(inst_cost_fn, "__self__", None)
    return owner.grid() if isinstance(owner, NavigationCost) else None


def cost_grid_key(inst_cost_fn):
    """What identifies that map in a controller's context key (NavigationCost.grid_key: kept between ticks), or None."""
    owner = getattr(inst_cost_fn, "__self__", None)
    return owner.grid_key() if isinstance(owner, NavigationCost) else None


def _probe_quadcos(fn):
    pts = torch.tensor([[0.3, 0.0], [0.0, 1.7], [2.1, -0.4], [-1.2, 3.3], [5.9, -7.1], [3.14159, 0.5]])
    try:
        out = torch.as_tensor(fn(pts)).reshape(-1).double()
    except Exception:
        return None
    if out.numel() != pts.shape[0]:
        return None
    a = ((pts[:, 0].cos() - 1) ** 2).double()
    b = (pts[:, 1] ** 2).double()
    A = torch.stack([a, b], dim=1)
    sol = torch.linalg.lstsq(A, out.unsqueeze(1)).solution.reshape(-1)
    if torch.allclose(A @ sol, out, rtol=1e-6, atol=1e-6):
        snap = lambda v: float('%.6g' % float(v))  # probing in fp32 leaves ~1e-8 noise on the fitted weights
        return snap(sol[0]), snap(sol[1])
    return None


def recognise(model, inst_cost_fn, term_cost_fn):
    """-> dict of dust_config cost fields, or raise NotImplementedError."""
    fam = getattr(model, "family", None)
    if fam == "pendulum":
        owner = getattr(inst_cost_fn, "__self__", None)
        if isinstance(owner, PendulumQuadCos):
            w = (owner.w_cos, owner.w_vel)
        else:
            w = _probe_quadcos(inst_cost_fn) if inst_cost_fn is not None else None
        if w is None:
            raise NotImplementedError("inst_cost_fn is not of the form w_cos (cos th - 1)^2 + w_vel thd^2: no HIP kernel for it "
                                      "(dust_amd has no CPU fallback)")
        wt = _probe_quadcos(lambda s: term_cost_fn(s)) if term_cost_fn is not None else None
        if wt is None or abs(wt[0] - w[0]) > 1e-6 * max(1, abs(w[0])) or abs(wt[1] - w[1]) > 1e-6 * max(1, abs(w[1])):
            raise NotImplementedError("term_cost_fn must equal the instantaneous pendulum cost (demo/pendulum_example.py:27-28)")
        return dict(w_cos=w[0], w_vel=w[1])
    if fam == "particle":
        ok = (getattr(inst_cost_fn, "__func__", None) is type(model).default_inst_cost and
              getattr(term_cost_fn, "__func__", None) is type(model).default_term_cost)
        if not ok:
            raise NotImplementedError("Particle needs model.default_inst_cost / model.default_term_cost (no CPU fallback)")
        m = inst_cost_fn.__self__
        return dict(target=tuple(float(v) for v in m.target), w_state=tuple(float(v) for v in m.w_state),
                    w_term=tuple(float(v) for v in m.w_term), w_ctrl=tuple(float(v) for v in m.w_ctrl), w_obs=float(m.w_obs))
    if fam == "skid_steer":
        owner = getattr(inst_cost_fn, "__self__", None)
        if not isinstance(owner, QuadraticCost) or getattr(term_cost_fn, "__self__", None) is not owner:
            raise NotImplementedError("SkidSteerRobot runs with dust_amd.costs.QuadraticCost(...).inst_cost / .term_cost (the reference ships "
                                      "no cost for this model; an opaque callable cannot run on the device and there is no CPU fallback)")
        if owner.goal.numel() != 5 or owner.w_state.numel() != 5 or owner.w_term.numel() != 5:
            raise ValueError("QuadraticCost for SkidSteerRobot needs 5 state entries (x, y, theta, v, omega)")
        wc = owner.w_ctrl if owner.w_ctrl is not None else torch.zeros(2)
        out = dict(goal=tuple(float(v) for v in owner.goal), w_quad_state=tuple(float(v) for v in owner.w_state),
                   w_quad_term=tuple(float(v) for v in owner.w_term), w_quad_ctrl=tuple(float(v) for v in wc))
        if type(owner) is QuadraticCost:
            return out
        # A subclass adds terms the quadratic kernels do not evaluate: only the navigation family's own methods are known
        if (type(owner) is not NavigationCost or getattr(inst_cost_fn, "__func__", None) is not NavigationCost.inst_cost or
                getattr(term_cost_fn, "__func__", None) is not NavigationCost.term_cost):
            raise NotImplementedError("%s extends QuadraticCost: the device evaluates QuadraticCost and NavigationCost themselves, and "
                                      "whatever a subclass adds would be dropped silently (no CPU fallback)" % type(owner).__name__)
        if not 0.0 <= owner.w_obs < float("inf"):
            raise ValueError("NavigationCost(w_obs=%r): a finite weight >= 0" % (owner.w_obs,))
        if owner.w_obs != 0.0 and owner.obst_map is None:
            raise ValueError("NavigationCost(w_obs=%g) without obst_map: the obstacle term reads obst_map.get_collisions "
                             "(particle.py:172-175, obstacle_map.py:64-93)" % owner.w_obs)
        out["w_obs"] = owner.w_obs
        if owner.obst_map is not None:
            out["cell_size"] = float(owner.obst_map.cell_size)
        return out
    if fam == "cartpole":
        owner = getattr(inst_cost_fn, "__self__", None)
        if isinstance(owner, NavigationCost):
            raise NotImplementedError("NavigationCost on CartPoleModel: the obstacle term reads the position plane states[..., 0:2] "
                                      "(particle.py:174), which the cart-pole's state (x, x_d, theta, theta_d) does not have")
        if not isinstance(owner, QuadraticCost) or getattr(term_cost_fn, "__self__", None) is not owner:
            raise NotImplementedError("CartPoleModel runs with dust_amd.costs.QuadraticCost(...).inst_cost / .term_cost (an opaque "
                                      "callable cannot run on the device and there is no CPU fallback)")
        if owner.goal.numel() != 4 or owner.w_state.numel() != 4 or owner.w_term.numel() != 4:
            raise ValueError("QuadraticCost for CartPoleModel needs 4 state entries (x, x_d, theta, theta_d)")
        if owner.w_ctrl is not None and owner.w_ctrl.numel() != 1:
            raise ValueError("QuadraticCost for CartPoleModel needs 1 control weight")
        wc = owner.w_ctrl if owner.w_ctrl is not None else torch.zeros(1)
        return dict(goal=tuple(float(v) for v in owner.goal), w_quad_state=tuple(float(v) for v in owner.w_state),
                    w_quad_term=tuple(float(v) for v in owner.w_term), w_quad_ctrl=tuple(float(v) for v in wc))
    raise NotImplementedError("model family %r has no HIP kernel" % (fam,))
