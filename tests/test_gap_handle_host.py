"""Host-side checks of the solver handle's in-loop duality gap (mmw_set_gap / mmw_read_gap / mmw_gap_checks, `mmw(gap_log=...)`,
`convergence.convergence`): the check schedule and every refusal that needs no device."""
import numpy as np
import pytest

from sig_sdp_mmw_amd import _lib
from sig_sdp_mmw_amd.convergence import convergence
from sig_sdp_mmw_amd.graphs import er_contention_graph
from sig_sdp_mmw_amd.mmw import mmw


def test_check_schedule_at_the_default_cap():
    want = [10, 20, 30, 40, 50, 62, 77, 96, 120, 150, 187, 233, 291, 363, 453, 566, 600]
    assert _lib.gap_checks(600, 0) == want
    assert _lib.gap_checks(10003) == want


def test_check_schedule_of_small_instances_and_small_caps():
    assert _lib.gap_checks(7) == [7]
    assert _lib.gap_checks(192, 10) == [10]
    assert _lib.gap_checks(11) == [10, 11]
    assert _lib.gap_checks(2000, 1024)[-1] == 1024


def test_a_cap_beyond_the_tridiagonal_is_refused():
    with pytest.raises(_lib.MMWError):
        _lib.gap_checks(2000, 1025)
    with pytest.raises(_lib.MMWError):
        _lib.gap_checks(0)


def test_host_only_handle_refuses_the_gap_with_err_state():
    s = _lib.Solver(4, er_contention_graph(30, 0.2, 0), 5, 0.1, device=-1)
    with pytest.raises(_lib.MMWError) as e:
        s.set_gap()
    assert "-3" in str(e.value) or "host-only" in str(e.value), str(e.value)
    L = _lib.lib()
    assert L.mmw_set_gap(s._h, 1, 0, 0) == -3
    assert L.mmw_set_gap(s._h, 1, 1025, 0) == -3  # (the handle's kind is looked at first)
    out = np.empty(4)
    assert L.mmw_read_gap(s._h, _lib._pd(out), 4) == -3
    s.close()


def test_class_keyword_is_checked():
    with pytest.raises(ValueError):
        mmw(gap_log="bogus")
    a = mmw(log_gap=True, gap_log="loop", device=-1)
    assert a.gap_log == "loop" and a.sibling().gap_log == "loop"
    assert mmw().gap_log == "call"


@pytest.mark.parametrize("Z", [0, 31, -2])
def test_convergence_rejects_a_slot_count_outside_the_instance(Z):
    with pytest.raises(ValueError):
        convergence(Z, er_contention_graph(30, 0.2, 0), 5, 0.1, device=-1)
