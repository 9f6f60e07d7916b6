"""Closed-loop control periods per second of the dual loop over an AMPPI controller, three forms:
  (a) the hand composition from public calls that predate DualAMPPI (model.params_dist = mpf.prior; controller.update_actions;
      controller.roll(1); mpf.optimize): the parameter rows of every tick come to the host and go back;
  (b) DualAMPPI(fused=False): the same composition behind the class;
  (c) DualAMPPI(fused=True): one C call per period, the rows drawn inside the tick's kernel.
Shapes: Pendulum (length, mass) and skid-steer with a NavigationCost (x_icr, axial_distance), H = 20, params_sampling="extended",
S in {1024, 16384}, 256 filter particles, 20 filter steps, Silverman bandwidths; the plant is the host model with other parameters.  A
period ends with the action on the host, so every timed window ends synchronised.  Each form runs in a child process of its own under a
time limit; a form that fails or runs out of time ends the run.  Every figure is taken twice (two windows, alternating over the shapes).

    python tools/amppi_dual_time.py [--periods 200] [--forms abc] [--root DIR]    (--root: time form (a) on another checkout's package)"""
import argparse
import os
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIMIT = 240  # seconds per form


def build(shape, S, root):
    sys.path.insert(0, root)
    import torch

    from dust_amd.controllers import AMPPI
    from dust_amd.costs import NavigationCost, PendulumQuadCos
    from dust_amd.inference import MPF, GaussianLikelihood
    from dust_amd.models import PendulumModel, SkidSteerRobot
    from dust_amd.utils.obstacle_map import generate_obstacle_map, get_obst_preset

    torch.manual_seed(0)
    H, Mp = 20, 256
    if shape == "pendulum":
        model = PendulumModel(uncertain_params=("length", "mass"))
        plant = PendulumModel(length=1.1, mass=0.9)
        cost = PendulumQuadCos()
        start, lam, a_cov, lr, obs = torch.tensor([3.0, 0.0]), 100.0, 4.0 * torch.eye(1), 1e-3, 0.1
        x0 = torch.tensor([1.0, 1.0]) * (1.0 + 0.1 * torch.randn(Mp, 2))
        init = None
    else:
        om = generate_obstacle_map(map_dim=(22, 22), obst_list=get_obst_preset("grid_6x6", obst_width=1.0), cell_size=0.1, map_type="direct")
        model = SkidSteerRobot(delta_t=0.1, uncertain_params=("x_icr", "axial_distance"), min_wheel_speed=-3.0, max_wheel_speed=3.0)
        plant = SkidSteerRobot(delta_t=0.1, x_icr=0.25, axial_distance=0.5, min_wheel_speed=-3.0, max_wheel_speed=3.0)
        cost = NavigationCost((2.6, 2.9, 0.0, 0.0, 0.0), (1.0, 1.0, 0.0, 0.0, 0.0), (20.0, 20.0, 0.0, 0.0, 0.0), None, obst_map=om, w_obs=20.0)
        start, lam, a_cov, lr, obs = torch.tensor([-2.9, -2.6, 0.6, 0.0, 0.0]), 5.0, torch.eye(2), 2e-6, 0.05
        x0 = torch.tensor([0.2, 0.475]) * (1.0 + 0.1 * torch.randn(Mp, 2))
        init = 1.5 * torch.ones(H, 2)
    ctrl = AMPPI(model.observation_space, model.action_space, H, S, lambda_=lam, a_cov=a_cov, inst_cost_fn=cost.inst_cost, term_cost_fn=cost.term_cost,
                 params_sampling="extended", init_actions=init, seed=0)
    ctrl.return_rollouts = False
    mpf = MPF(init_particles=x0, likelihood=GaussianLikelihood(initial_obs=start, obs_std=obs, model=model, log_space=False),
              optimizer_class=torch.optim.SGD, lr=lr, bw=None, bw_scale=1.0)
    return ctrl, model, mpf, plant, start


def child(form, periods, root):
    import torch

    shapes = [(sh, S) for sh in ("pendulum", "skid_nav") for S in (1024, 16384)]
    loops = []
    for sh, S in shapes:
        ctrl, model, mpf, plant, start = build(sh, S, root)
        step = lambda x, u, p=plant: p.step(x.reshape(1, -1), u.reshape(1, -1))
        if form == "a":
            def period(state, ctrl=ctrl, model=model, mpf=mpf, step=step):
                model.params_dist = mpf.prior
                ctrl.update_actions(model, state)
                action = ctrl.a_seq[0]
                ctrl.roll(1)
                new = step(state, action)
                mpf.optimize(action.squeeze() if action.numel() == 1 else action, new, bw=None, n_steps=20)
                return new
        else:
            from dust_amd.controllers import DualAMPPI

            loop = DualAMPPI(ctrl, model, mpf, mpf_bw=None, mpf_steps=20, fused=form == "c", seed=0)
            period = lambda state, loop=loop, step=step: loop.tick(state, step)[1]
        loops.append([sh, S, period, start.reshape(1, -1), start.reshape(1, -1)])
    for lp in loops:  # warm every shape up: code objects, contexts, the first filter update
        for _ in range(20):
            lp[4] = lp[2](lp[4])
    for window in range(2):
        for lp in loops:
            lp[4] = lp[3]
            t0 = time.perf_counter()
            for _ in range(periods):
                lp[4] = lp[2](lp[4])  # (the action came to the host inside: the stream is drained)
            dt = (time.perf_counter() - t0) / periods
            ok = bool(torch.isfinite(lp[4]).all())
            print("form %s  %-8s S %5d  window %d: %8.1f us per period (%7.0f periods/s)%s"
                  % (form, lp[0], lp[1], window, 1e6 * dt, 1.0 / dt, "" if ok else "  NON-FINITE STATE"), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--periods", type=int, default=200)
    ap.add_argument("--forms", default="abc")
    ap.add_argument("--root", default=HERE)
    ap.add_argument("--child", default=None)
    a = ap.parse_args()
    if a.child:
        child(a.child, a.periods, os.path.abspath(a.root))
        return 0
    for form in a.forms:
        cmd = [sys.executable, os.path.abspath(__file__), "--child", form, "--periods", str(a.periods), "--root", a.root]
        try:
            rc = subprocess.run(cmd, timeout=LIMIT).returncode
        except subprocess.TimeoutExpired:
            print("form %s: no result within %d s - stopping" % (form, LIMIT), flush=True)
            return 124
        if rc != 0:
            print("form %s: exit status %d - stopping" % (form, rc), flush=True)
            return rc
    return 0


if __name__ == "__main__":
    sys.exit(main())
