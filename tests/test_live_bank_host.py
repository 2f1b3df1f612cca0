"""The tracker bank's host side: aar_tracker_bank_params_validate, the size-versioned stats struct and the answer without a
device.  No GPU needed."""
import ctypes as C

import numpy as np
import pytest

import aar
import smooth_cases as sc


def _sols(n):
    ds = aar.synth(2, num_frames=2)
    return [ds] * n


def _refused(word, solutions, **kw):
    with pytest.raises(aar.AarError) as e:
        aar.tracker_bank_params_validate(solutions, **kw)
    assert e.value.code == aar.AAR_ERR_INVALID and word in str(e.value), str(e.value)
    return str(e.value)


def test_symbols_are_exported():
    L = aar.lib()
    for name in aar.SYMBOLS:
        if name.startswith("aar_tracker_bank_"):
            assert hasattr(L, name), name
    assert sum(n.startswith("aar_tracker_bank_") for n in aar.SYMBOLS) == 11 and aar.TRACKER_BANK_MAX_MEMBERS == 1024


def test_member_counts():
    aar.tracker_bank_params_validate(_sols(1))
    aar.tracker_bank_params_validate(_sols(aar.TRACKER_BANK_MAX_MEMBERS))
    _refused("n_members = 0", _sols(1), n_members=0)
    _refused("n_members = -1", _sols(1), n_members=-1)
    _refused("n_members = %d" % (aar.TRACKER_BANK_MAX_MEMBERS + 1), _sols(aar.TRACKER_BANK_MAX_MEMBERS + 1))


def test_null_entry_and_bad_member_are_named():
    s = _sols(4)
    _refused("member 1: null solution", [s[0], None, s[2], s[3]])
    bad = sc.copy_of(s[2], marker_size=float("nan"))
    msg = _refused("member 2: ", [s[0], s[1], bad, s[3]])
    assert "marker_size" in msg
    x = np.array(s[0].x_full)
    x[3] = np.inf
    msg = _refused("member 3: ", [s[0], s[1], s[2], sc.copy_of(s[3], x_full=x)])
    assert "x_full[3]" in msg
    aar.tracker_bank_params_validate(s)


def test_params_rules_hold_for_the_bank():
    s = _sols(3)
    msg = _refused("struct_size", s, struct_size=8)
    assert "member 0: " in msg
    _refused("needs smooth = 1", s, lag=2)
    _refused("sigma_rot", s, lag=2, smooth=True, sigma_rot=0.0, sigma_trans=0.1)
    _refused("anchor_mode", s, lag=0, smooth=True, sigma_rot=0.1, sigma_trans=0.1, anchor="marginal")
    aar.tracker_bank_params_validate(s, lag=15, smooth=True, sigma_rot=0.1, sigma_trans=0.1, anchor="marginal", covariance=True)


def test_members_may_differ_in_size():
    a, b = aar.synth(2, num_frames=2), aar.synth(2, num_cams=3, num_markers=6, num_frames=2, min_view_cos=0.3)
    assert (a.num_cams, a.num_markers) != (b.num_cams, b.num_markers)
    aar.tracker_bank_params_validate([a, b, a])


def test_stats_struct_size_and_null_arguments():
    L = aar.lib()
    st = aar.CTrackerBankStats()
    st.struct_size = C.sizeof(aar.CTrackerBankStats)
    assert C.sizeof(aar.CTrackerBankStats) == 56
    assert L.aar_tracker_bank_get_stats(None, C.byref(st)) == aar.AAR_ERR_INVALID                  # no bank
    assert L.aar_tracker_bank_size(None) == 0
    assert L.aar_tracker_bank_reset(None) == aar.AAR_ERR_INVALID
    assert L.aar_tracker_bank_window(None, 0, None, None, None, None, None, None, None) == aar.AAR_ERR_INVALID
    assert L.aar_tracker_bank_push(None, 0.0, None, None, None, None, None, None, None) == aar.AAR_ERR_INVALID
    L.aar_tracker_bank_destroy(None)                                                                # harmless


@pytest.mark.skipif(aar.device_count() > 0, reason="a HIP device is present: creation succeeds (tests/test_gpu_live_bank.py)")
def test_create_without_a_device_answers_no_device():
    with pytest.raises(aar.AarError) as e:
        aar.TrackerBank(_sols(2))
    assert e.value.code == aar.AAR_ERR_NO_DEVICE
    # ... after validation: a bad bank is AAR_ERR_INVALID also here
    with pytest.raises(aar.AarError) as e:
        aar.TrackerBank(_sols(2), lag=3)
    assert e.value.code == aar.AAR_ERR_INVALID
    L = aar.lib()
    assert L.aar_tracker_bank_enable_detections(None, None) == aar.AAR_ERR_NO_DEVICE
