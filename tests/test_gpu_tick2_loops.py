"""The hot loops of the one-launch tick (dust_amd/csrc/tick2.hpp) may be re-scheduled - fewer instructions, less exposed latency - but
not re-ordered: the Stein pass's key rows ping-pong between two register pairs over a trip of four steps, and whatever is tried next on
the rollout waves' weighted sums (grouped LDS reads, `same_w` outside the loop) or on K x score (rows requested in front of barrier B4)
must keep every operation and the order of every sum: every output keeps every bit.  The fixtures (tests/golden/tick2_loops_<case>.npz,
written by tools/record_tick2_golden.py --cases tick2_loops_cases) hold the results of the library as it was BEFORE the Stein loop
was rewritten (commit 4bddf0b), three ticks per case; ticks 2-3 are tick2 launches.  `costs` always, the [N, D] arrays at N >= 1000 and
whatever else has more than 16 384 elements are held as one CRC-32 per particle row."""
import numpy as np
import pytest

import tick2_loops_cases as cases
from test_gpu_serve import _loop

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", list(cases.CASES))
def test_hot_loops_keep_every_bit(name):
    """What each case reaches is written beside it in tests/tick2_loops_cases.py: the unmasked and the masked Stein instance with keys
    ending inside and far in front of the last trip, sample counts that fill, overfill and do not fill a group of eight (S = 40, 45, 96,
    200), the omega body (alpha * temp != 1), full 32-column rows in both kernel modes, caller-supplied noise."""
    want = np.load(cases.golden_path(name))
    got, stats = cases.run_case(name)
    assert stats["tick2"] == cases.tick2_launches(name) and stats["replayed"] == 0, stats
    assert sorted(got) == sorted(want.files)
    for k in sorted(got):
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, k
        assert np.array_equal(got[k], want[k]), (k, int((got[k] != want[k]).sum()))


def test_served_loop_keeps_every_bit_with_the_ping_pong_stein_loop():
    """8 closed-loop ticks of three iterations served (armed launches) against the same loop unserved."""
    model, N, S, H, iters = "pendulum", 64, 128, 15, 3
    a, _ = cases.make(model, N, S, H)
    ra, tha, ama, ca, sa = _loop(a, model, iters, 8, serve=False)
    a.close()
    b, _ = cases.make(model, N, S, H)
    rb, thb, amb, cb, sb = _loop(b, model, iters, 8, serve=True)
    b.close()
    for t, ((a0, p0, s0), (a1, p1, s1)) in enumerate(zip(ra, rb)):
        assert np.array_equal(s0, s1), t
        assert np.array_equal(a0, a1), (t, np.abs(a0 - a1).max())
        assert np.array_equal(p0, p1), t
    assert np.array_equal(tha, thb) and np.array_equal(ama, amb) and np.array_equal(ca, cb)
    assert sa["served"] == 0 and sa["replayed"] == 0, sa
    assert sb["served"] == 8 and sb["replayed"] == 0, sb
