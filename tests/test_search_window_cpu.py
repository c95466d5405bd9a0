"""CPU: the window policy of the SNR-offset search (csrc/snr_window.h: win_first_lo / win_next_lo), restated in
profiles/search_window_sim.py, on the oracle's spare-bit curves - as tests/test_search_policy.py does for the three-offset
policy.  Which offsets are costed never changes a result; the policy must end where the reference's own loop ends, from any
start value, in a bounded number of sweeps, and a transcode's hint must pay."""
import os
import sys

import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles"))

STARTS = (40, 0, 63, 7, 11, 12, 25)


@pytest.fixture(scope="module")
def sims():
    import search_sim
    import search_window_sim
    fresh = search_sim.curves(6, seed=5)
    second = search_sim.curves(3, seed=6, second_gen=True, with_source=True)
    return search_sim, search_window_sim, fresh, second


@pytest.mark.parametrize("hinted", [False, True])
def test_the_window_policy_replays_the_reference(sims, hinted):
    sim, win, fresh, second = sims
    cases = [(c, 16 * sim.reference(c, 40)[0] + sim.reference(c, 40)[1]) for c in fresh] + list(second)
    for c, g_hint in cases:
        for start in STARTS:
            sweeps, got = win.run(c, start, hint=g_hint if hinted else None)
            assert got == sim.reference(c, start), (start, hinted)
            assert 1 <= sweeps <= 12, (start, hinted, sweeps)


def test_hinted_second_generation_frames_need_fewer_sweeps(sims):
    sim, win, fresh, second = sims
    window = sum(win.run(c, 40, hint=g)[0] for c, g in second)
    probe = sum(sim.run(c, 40, "probe", hint=g)[0] for c, g in second)
    assert window < probe, (window, probe)
