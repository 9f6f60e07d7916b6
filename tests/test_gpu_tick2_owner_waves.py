"""The owner lanes of the one-launch tick (dust_amd/csrc/tick2.hpp) ride rollout waves 0-1 instead of pair waves 8-9, and pair waves
8-9 draw the second noise share of waves 0-1 for them.  Only the wave that hosts an operation changed, no operation and no order:
every output must keep every bit.  The fixtures (tests/golden/tick2_ow_<case>.npz, written by tools/record_tick2_golden.py) hold the
results of the library as it was BEFORE the move, three ticks per case; ticks 2-3 are the tick2 ticks."""
import numpy as np
import pytest

import tick2_ow_cases as cases
from test_gpu_serve import _loop
from test_gpu_tick2 import _make

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", list(cases.CASES))
def test_owner_waves_keep_every_bit(name):
    """n64_s128_h15_it3: both stand-in draws over two waves per particle, three generations.  n96_s64_h20_it3_adam: S = 64 - odd rollout
    waves own no samples; masked keys; optimiser moments in the owner lanes' registers.  n64_s96_h12_m4_it2: a ragged second wave of
    samples, coefficients from wave 11.  n64_s128_h16_it1_eps: the one-iteration go-word wait in the wave that also publishes.
    n64_s128_h16_it2_eps: caller-supplied noise staged with waves 0-1 arriving late.  n128_s128_h30_it2_imq_wprior: the other kernel
    mode and the mixture tail.  particle_n64_s64_h12_it2_rollmean: D = 24, d_a = 2, the roll's half-wave sums on waves 0-1.
    n64_h15_adam_opt2_fwd: both COMMIT exits and the launch without iterations."""
    want = np.load(cases.golden_path(name))
    got, stats = cases.run_case(name)
    assert stats["tick2"] == cases.tick2_launches(name) and stats["replayed"] == 0, stats
    assert sorted(got) == sorted(want.files)
    for k in sorted(got):
        assert got[k].shape == want[k].shape and np.array_equal(got[k], want[k]), (k, float(np.abs(got[k] - want[k]).max()))


def test_served_loop_keeps_every_bit_with_owner_lanes_on_rollout_waves():
    """An armed launch: waves 0-1 wait for the mailbox in front of their rollouts and hold the owner lanes' registers meanwhile.
    8 closed-loop ticks served against the same loop unserved."""
    model, N, S, H, iters = "pendulum", 64, 128, 15, 3
    a, _ = _make(model, N, S, H)
    ra, tha, ama, ca, sa = _loop(a, model, iters, 8, serve=False)
    a.close()
    b, _ = _make(model, N, S, H)
    rb, thb, amb, cb, sb = _loop(b, model, iters, 8, serve=True)
    b.close()
    for t, ((a0, p0, s0), (a1, p1, s1)) in enumerate(zip(ra, rb)):
        assert np.array_equal(s0, s1), t
        assert np.array_equal(a0, a1), (t, np.abs(a0 - a1).max())
        assert np.array_equal(p0, p1), t
    assert np.array_equal(tha, thb) and np.array_equal(ama, amb) and np.array_equal(ca, cb)
    assert sa["served"] == 0 and sa["replayed"] == 0, sa
    assert sb["served"] == 8 and sb["replayed"] == 0, sb
