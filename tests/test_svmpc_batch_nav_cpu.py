"""The navigation cost in the batched SVMPC tick without a device: the two new kernel instances and their register allocation beside the
eight that were there, `BatchSVMPC` / `BatchDualSVMPC` over a `NavigationCost` controller (construction and the refusals that stay), and
the box against the navigation fixtures' scenarios."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import __graft_entry__ as entry
import skid_nav_cases as cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURES = ("nominal", "ragged", "p3_log", "scalar", "offmap", "bigmap")  # tests/test_gpu_svmpc_batch_nav.py runs these through the batch


@pytest.fixture(scope="module")
def built():
    return entry.build()


@pytest.fixture(scope="module")
def kernels(built, tmp_path_factory):
    """the method of test_svmpc_batch_cpu.py test_batch_kernels_do_not_spill: name -> (spilled VGPRs, private segment, VGPRs) from the
    gfx950 code object's metadata"""
    llvm = "/opt/rocm/lib/llvm/bin"
    if not (os.path.exists(llvm + "/llvm-objdump") and os.path.exists(llvm + "/llvm-readelf")):
        pytest.skip("llvm-objdump / llvm-readelf not available")
    tmp = str(tmp_path_factory.mktemp("co"))
    shutil.copy(built, os.path.join(tmp, "l.so"))
    subprocess.run([llvm + "/llvm-objdump", "--offloading", "l.so"], cwd=tmp, check=True, capture_output=True)
    co = [f for f in os.listdir(tmp) if "gfx950" in f]
    assert co, "no gfx950 code object in libdust_amd.so"
    notes = "".join(subprocess.run([llvm + "/llvm-readelf", "--notes", f], cwd=tmp, check=True, capture_output=True, text=True).stdout for f in co)
    out = {}
    for m in re.finditer(r"\.name:\s+(\S+)\n(.*?)\.wavefront_size", notes, re.S):
        blk = m.group(2)
        out[m.group(1)] = (int(re.search(r"\.vgpr_spill_count:\s+(\d+)", blk).group(1)),
                           int(re.search(r"\.private_segment_fixed_size:\s+(\d+)", blk).group(1)),
                           int(re.search(r"\.vgpr_count:\s+(\d+)", blk).group(1)))
    return out


def test_navigation_instances_exist_once_and_do_not_spill(kernels):
    for name in ("svmpc_skid_nav_batch_kernel", "svmpc_skid_nav_prior_batch_kernel"):
        mine = {k: v for k, v in kernels.items() if name in k}
        assert len(mine) == 1, (name, sorted(mine))
        (spill, scratch, vgprs), = mine.values()
        assert spill == 0 and scratch == 0 and vgprs <= 256, (name, spill, scratch, vgprs)  # (512 lanes per workgroup: 256 VGPRs per lane)


def test_the_eight_plain_instances_are_still_there(kernels):
    for name in ("svmpc_batch_kernel", "svmpc_prior_batch_kernel"):
        mine = {k: v for k, v in kernels.items() if name in k}
        assert len(mine) == 4, (name, sorted(mine))
        assert not any("nav" in k for k in mine)
        for k, (spill, scratch, vgprs) in mine.items():
            assert spill == 0 and scratch == 0 and vgprs <= 256, (k, spill, scratch, vgprs)


def _parts(N=4, H=6, S=16, M=3, a_cov=None, p_cov=None, sampling=True, **ctrl_kw):
    import torch

    from dust_amd.controllers import MultiDISCO
    from dust_amd.costs import NavigationCost
    from dust_amd.inference import ExponentiatedUtility, get_gmm
    from dust_amd.models import SkidSteerRobot
    from dust_amd.utils.obstacle_map import ObstacleMap

    s = cases.ROLLOUT_BY_TAG["nominal"]
    om = ObstacleMap(list(s["map_dim"]), s["cell"])
    om.map = cases.make_map(s).astype(np.float64)
    cost = NavigationCost(cases.GOAL, cases.W_STATE, cases.W_TERM, torch.tensor(cases.W_CTRL), obst_map=om, w_obs=s["w_obs"])
    model = SkidSteerRobot(delta_t=s["dt"], uncertain_params=("x_icr", "wheel_radius"), min_wheel_speed=s["bounds"][0], max_wheel_speed=s["bounds"][1])
    ctrl = MultiDISCO(model.observation_space, model.action_space, H, N, S, a_cov=torch.eye(2) if a_cov is None else a_cov, inst_cost_fn=cost.inst_cost,
                      term_cost_fn=cost.term_cost, params_sampling=sampling, params_samples=M, **ctrl_kw)
    prior = get_gmm(torch.zeros(N, H, 2), torch.ones(N), torch.eye(2) if p_cov is None else p_cov)
    lik = ExponentiatedUtility(alpha=1.0, n_samples=S, controller=ctrl, model=model)
    return torch.zeros(N, H, 2), prior, lik, cost


class _Filter:
    """what BatchDualSVMPC's constructor reads of an MPF ahead of any device call"""

    class _Dev:
        Mp, P = 16, 2

    def __init__(self):
        self.draw_source, self._dev = None, self._Dev()


def test_batch_classes_construct_over_a_navigation_cost_without_a_device():
    import torch
    import torch.distributions as dist

    from dust_amd.controllers import BatchDualSVMPC
    from dust_amd.inference import BatchSVMPC
    from dust_amd.kernels import IMQ, RBFKernel

    th, prior, lik, cost = _parts()
    for kernel in (None, RBFKernel(), IMQ(0.7)):
        b = BatchSVMPC(3, th, prior, lik, kernel=kernel, optimizer_class=torch.optim.SGD, lr=0.5, seeds=(7, 7, 9))
        assert b.n_envs == 3 and tuple(b.theta.shape) == (3, 4, 6, 2) and b._batch is None and lik.controller._ctx is None
    loop = BatchDualSVMPC(b, _Filter(), mpf_steps=7, seed=5)
    assert loop.n_envs == 3 and loop._mb is None and b._batch is None and lik.controller._ctx is None
    # what the batch will hand to the device: the family's weight, the map's cell size and the map's identity (still no device)
    pd = dist.Independent(dist.Uniform(torch.tensor([0.1, 0.05]), torch.tensor([0.3, 0.08])), 1)
    cfg = lik.controller._config(lik.model, pd)
    s = cases.ROLLOUT_BY_TAG["nominal"]
    assert cfg["model"] == "skid_steer" and cfg["w_obs"] == s["w_obs"] and cfg["cell_size"] == pytest.approx(s["cell"]) and "nav_map" in cfg
    assert cfg["kernel"] == "IMQ" and cfg["ctrl_penalty"] == 1.0 and lik.controller._ctx is None
    assert np.array_equal(cost.grid(), cases.make_map(s))
    for cls in (BatchSVMPC, BatchDualSVMPC):
        assert "NavigationCost" in cls.__doc__, cls.__name__


def test_constructors_still_refuse_what_lies_outside_the_box():
    import torch

    from dust_amd.controllers import BatchDualSVMPC
    from dust_amd.inference import BatchSVMPC
    from dust_amd.kernels import RBF, iid_mp
    from dust_amd.utils.utf import MerweScaledUTF

    th, prior, lik, _ = _parts()
    for kernel in (iid_mp(base_kernel=RBF(bandwidth=-1), ctrl_dim=2, indep_controls=True), iid_mp(base_kernel=RBF(), indep_controls=False)):
        with pytest.raises(NotImplementedError, match="K1 .* IMQ"):
            BatchSVMPC(3, th, prior, lik, kernel=kernel)
    with pytest.raises(NotImplementedError, match="resample"):
        BatchSVMPC(3, th, prior, lik, roll_strategy="resample")
    th_s, prior_s, lik_s, _ = _parts(sampling=MerweScaledUTF(n=2))
    with pytest.raises(NotImplementedError, match="sigma-point"):
        BatchSVMPC(3, th_s, prior_s, lik_s)
    th_c, prior_c, lik_c, _ = _parts(ctrl_penalty=0.6)
    with pytest.raises(NotImplementedError, match="ctrl_penalty = 1"):
        BatchSVMPC(3, th_c, prior_c, lik_c)
    full = torch.tensor(cases.FULL_COV)
    for a_cov, p_cov in ((full, None), (None, full)):
        th_f, prior_f, lik_f, _ = _parts(a_cov=a_cov, p_cov=p_cov)
        with pytest.raises(NotImplementedError, match="diagonal covariances"):
            BatchSVMPC(3, th_f, prior_f, lik_f)
    th_0, prior_0, lik_0, _ = _parts(sampling=None)
    with pytest.raises(ValueError, match="samples dynamics parameters"):
        BatchDualSVMPC(BatchSVMPC(3, th_0, prior_0, lik_0, optimizer_class=torch.optim.SGD, lr=0.5), _Filter())


def test_navigation_fixtures_lie_inside_the_box():
    by_tag = {s["tag"]: s for s in cases.ROLLOUTS}
    for tag in FIXTURES:
        s = by_tag[tag]
        assert s["kind"] == "disco", tag
        assert 1 <= s["N"] <= 64 and 1 <= s["S"] <= 1024 and 1 <= s["M"] <= 64 and 2 * s["H"] <= 128 and len(s["up"]) <= 4, tag
        assert s["ctrl_penalty"] == 1.0 and s["a_cov"] is None, tag  # (a_cov None: SIGMA_A^2 I, diagonal)
        g = dict(np.load(os.path.join(ROOT, "tests", "golden", cases.fixture_name(s) + ".npz"), allow_pickle=False))
        assert g["eps"].shape == (s["S"], s["N"], s["H"], 2) and g["costs"].shape == (s["S"], s["N"]), tag
        assert ("params" in g) == bool(s["up"]) and (not s["up"] or g["params"].shape == (s["M"], len(s["up"]))), tag
        for v in s["offs"]:
            assert "costs_off_" + v in g, (tag, v)
        for q in ("costs", "a_mat1", "a_mix"):
            assert "tol_" + q in g, (tag, q)
    # what the batch cannot take of the navigation scenarios is exactly what the GPU test leaves out
    out = {s["tag"] for s in cases.ROLLOUTS if s["kind"] != "disco" or s["ctrl_penalty"] != 1.0 or s["a_cov"] is not None}
    assert out == {"areg", "fullcov", "ut_p1", "ut_p3"} and out | set(FIXTURES) == set(cases.ROLLOUT_NAMES)
    words = {t: (np.prod(cases.map_cells(by_tag[t])) + 31) // 32 for t in FIXTURES}
    assert words["bigmap"] == 5000 > 4096 and all(w <= 4096 for t, w in words.items() if t != "bigmap")  # one fixture on the device-memory path
