"""The per-call inputs of the controller batches (csrc/dust_amd.hip BatchInputs: states and the active mask through two pinned slots).
A call that reads nothing back does not wait for its copy; the third such call in a row writes the slot of the first again, and must
find that copy done.  Bit for bit (np.array_equal): both sides run the same kernels on the same inputs."""
import numpy as np
import pytest

import amppi_cases as cases

pytestmark = pytest.mark.gpu

B, TICKS = 3, 4
MASKS = ((1, 1, 1), (1, 0, 1), (0, 1, 1), (1, 1, 0))


def _svmpc():
    from dust_amd import Context, _lib as L

    N, S, H = 4, 8, 4
    rng = np.random.default_rng(5)
    mu = rng.standard_normal((N, H, 1)).astype(np.float32)
    th = (mu + 2 * rng.standard_normal((N, H, 1))).astype(np.float32)
    proto = Context(model="pendulum", N=N, S=S, M=1, H=H, kernel="K1", optimizer="SGD", lr=2.0, sigma_a=2.0, sigma_p=2.0, seed=77)
    proto.set_theta(th)
    proto.set_prior(mu)
    proto.set_a_mat(th)
    batch = proto.svmpc_batch(B)
    proto.close()  # (the batch keeps its own copy)
    return batch, lambda b, st, on, out: b.tick(st, 1, active=on, want_outputs=out), lambda b: b.get(L.SVB_THETA)


def _amppi():
    from dust_amd import Context

    s = cases.A("inputs", "pendulum", 16, 4, "none", (), 900)
    proto = Context(**cases.context_kwargs(s))
    batch = proto.amppi_batch(B)
    proto.close()
    batch.set_a_seq(np.stack([cases.inputs(dict(s, seed=900 + b))["a_seq0"] for b in range(B)]))
    return batch, lambda b, st, on, out: b.update(st, None, None, active=on, want_outputs=out), lambda b: b.get_a_seq()


@pytest.mark.parametrize("kind", ["svmpc", "amppi"])
def test_back_to_back_calls_find_their_pinned_slot_free(kind):
    """Four ticks on device-drawn noise, each with its own states and its own mask: once without outputs, so that nothing synchronises
    while both slots go round twice, and once on a clone that reads its outputs - and so waits - after every tick"""
    batch, tick, result = _svmpc() if kind == "svmpc" else _amppi()
    twin = batch.clone()
    rng = np.random.default_rng(3)
    states = (np.array([3.0, 0.0], np.float32) + 0.3 * rng.standard_normal((TICKS, B, 2))).astype(np.float32)
    start = result(batch)
    for t in range(TICKS):
        tick(batch, states[t], MASKS[t], False)
    for t in range(TICKS):
        tick(twin, states[t], MASKS[t], True)
    got, want = result(batch), result(twin)
    twin.close()
    batch.close()
    assert np.array_equal(got, want)
    for b in range(B):  # (every environment ticked three times: the comparison is not one of untouched rows)
        assert not np.array_equal(got[b], start[b]), b
