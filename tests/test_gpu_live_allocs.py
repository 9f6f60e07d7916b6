"""Every handle type gives back what it took: device and pinned memory of dust_ctx, the controller batches, the dynamics filter and its
batch live in owners (csrc/devbuf.hpp) that count their blocks and bytes process-wide (dust_debug_live_allocs: a test hook, not part of
the C ABI).  Each scenario reads the two counters before and after - deltas, not zeros: fixtures of other modules may be alive - and
they must be equal.  Smallest shapes that reach the paths: Pendulum N = 8, S = 4, M = 1, H = 4 unless the path needs more."""
import ctypes as C
import gc

import numpy as np
import pytest

import amppi_cases

pytestmark = pytest.mark.gpu

STATE = np.array([3.0, 0.0], np.float32)


def _lib():
    from dust_amd import _lib as L

    lib = L.load()
    lib.dust_debug_live_allocs.argtypes = [C.POINTER(C.c_longlong)]
    lib.dust_debug_live_allocs.restype = C.c_int
    return lib


def live():
    """(blocks, bytes) the owners hold now"""
    gc.collect()
    out = (C.c_longlong * 2)()
    assert _lib().dust_debug_live_allocs(out) == 0
    return int(out[0]), int(out[1])


def _pendulum(N=8, S=4, H=4, kernel="K1", seed=11):
    from dust_amd import Context

    rng = np.random.default_rng(seed)
    mu = rng.standard_normal((N, H, 1)).astype(np.float32)
    th = (mu + 2 * rng.standard_normal((N, H, 1))).astype(np.float32)
    c = Context(model="pendulum", N=N, S=S, M=1, H=H, kernel=kernel, optimizer="SGD", lr=2.0, sigma_a=2.0, sigma_p=2.0, seed=seed)
    c.set_theta(th)
    c.set_prior(mu)
    c.set_a_mat(th)
    return c


def test_lone_context():
    """create, one tick, the phase-stamp hook where the build has it (-DDUST_STAMPS: its two blocks were never freed), destroy"""
    before = live()
    c = _pendulum()
    assert live()[0] > before[0]
    a_seq, pw = c.svmpc_tick(STATE, 2)
    assert np.isfinite(a_seq).all() and abs(float(pw.sum()) - 1.0) < 1e-4
    lib = _lib()
    if hasattr(lib, "dust_debug_stamps"):
        lib.dust_debug_stamps.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
        assert lib.dust_debug_stamps(c._h, 0, None) == 0  # (first call: allocates)
    c.close()
    assert live() == before


def test_clone_with_map_sigma_weights_and_pending_control_noise():
    from dust_amd import Context

    N, S, M, H = 8, 4, 3, 4
    before = live()
    grid = np.zeros((8, 8), np.float32)
    grid[5, 5] = 1.0
    c = Context(model="particle", N=N, S=S, M=M, H=H, kernel="K1", uncertain_params=("mass",), deterministic=False, noise_std=(0.1, 0.1),
                sigma_a=1.0, sigma_p=1.0, seed=5, grid=grid)
    c.set_param_weights(np.array([0.5, 0.25, 0.25], np.float32))
    rng = np.random.default_rng(5)
    c.set_ctrl_noise(rng.standard_normal((2, H, M * S * N, 2)).astype(np.float32))
    one = live()
    twin = c.clone()
    two = live()
    assert two[0] - one[0] == one[0] - before[0] and two[1] - one[1] == one[1] - before[1]  # the copy holds what its source holds
    twin.close()
    assert live() == one
    c.close()
    assert live() == before


def test_amppi_batch_and_its_clone():
    from dust_amd import Context

    B = 2
    before = live()
    s = amppi_cases.A("live", "pendulum", 16, 4, "none", (), 901)
    proto = Context(**amppi_cases.context_kwargs(s))
    batch = proto.amppi_batch(B)
    proto.close()
    twin = batch.clone()
    states = np.stack([STATE, STATE + 0.1]).astype(np.float32)
    for b in (batch, twin):
        a_seq = b.update(states, None, None)[2]
        assert np.isfinite(np.asarray(a_seq)).all()
    twin.close()
    batch.close()
    assert live() == before


def test_svmpc_batch_its_clone_and_an_episode():
    B = 2
    before = live()
    proto = _pendulum()
    batch = proto.svmpc_batch(B)
    proto.close()
    twin = batch.clone()
    states = np.stack([STATE, STATE + 0.1]).astype(np.float32)
    for b in (batch, twin):
        a_seq, pw = b.tick(states, 1)
        assert np.isfinite(a_seq).all() and np.isfinite(pw).all()
    held = live()
    xs, acts, pw, a_seq = batch.episode(states, 2, 1)  # (grows the plant rows and the records)
    assert np.isfinite(xs).all() and np.isfinite(acts).all()
    assert live()[0] > held[0]
    twin.close()
    batch.close()
    assert live() == before


def test_filter_its_batch_and_the_batch_clone():
    from dust_amd import MpfContext

    B, Mp = 2, 8
    before = live()
    rng = np.random.default_rng(3)
    x0 = (1.0 + 0.1 * rng.standard_normal((Mp, 2))).astype(np.float32)
    m = MpfContext(x0, STATE, model="pendulum", uncertain_params=("length", "mass"), obs_std=0.1, init_bw=0.15, lr=1e-3)
    mb = m.batch(B)
    twin = mb.clone()
    act, obs = np.array([0.5], np.float32), np.array([2.9, -0.4], np.float32)
    assert np.isfinite(m.optimize(act, obs, 0.15, 2)).all()
    for b in (mb, twin):
        gn, bw = b.optimize(np.stack([act] * B), np.stack([obs] * B), 0.15, 2)
        assert np.isfinite(gn).all()
    twin.close()
    mb.close()
    m.close()
    assert live() == before


def test_large_set_path_is_steady_and_returns_everything(monkeypatch):
    """Particle, N = 2048, D = 16 on the large-set path (run lists, far buffers, Gram matrix): below N * D = 65 536 the development
    switch DUST_PAIR_BIG=1 selects it (tests/test_gpu_pairwise_sizes.py does the same), and the prior has to alias the particles first.
    A second tick at the same shape allocates nothing."""
    from dust_amd import Context

    monkeypatch.setenv("DUST_PAIR_BIG", "1")
    N, S, H = 2048, 4, 8
    before = live()
    rng = np.random.default_rng(7)
    th = rng.standard_normal((N, H, 2)).astype(np.float32)
    c = Context(model="particle", N=N, S=S, M=1, H=H, kernel="K1", with_obstacle=False, sigma_a=1.0, sigma_p=1.0, seed=7)
    c.set_theta(th)
    c.set_a_mat(th)
    c.svmpc_update_prior()  # (the prior's means alias the particles from here on: the fused large-set pass)
    state = np.zeros(4, np.float32)
    created = live()
    a_seq, pw = c.svmpc_tick(state, 1)
    assert np.isfinite(a_seq).all() and np.isfinite(pw).all()
    first = live()
    n_units, js = C.c_int(0), C.c_int(0)
    lib = _lib()
    lib.dust_debug_pack_lists.argtypes = [C.c_void_p, C.c_int] + [C.c_void_p] * 6
    assert lib.dust_debug_pack_lists(c._h, -1, C.byref(n_units), C.byref(js), None, None, None, None) == 0, "the tick did not build run lists"
    assert first[0] >= created[0] + 8  # (five run lists, far rows / norms / flags, ...)
    c.svmpc_tick(state, 1)
    assert live() == first
    c.close()
    assert live() == before


def test_k2_context_with_its_transposed_ping_pong():
    before = live()
    c = _pendulum(N=64, kernel="K2")
    for _ in range(2):
        a_seq, pw = c.svmpc_tick(STATE, 2)
        assert np.isfinite(a_seq).all()
    c.close()
    assert live() == before
