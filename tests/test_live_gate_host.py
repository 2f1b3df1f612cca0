"""The gate of the live trackers: what needs no device -- the parameter checks of include/aar.h, the float64 restatement
(tests/live_gate_restated.py) against hand-worked lists, and the margin condition of every case of tests/live_gate_cases.py.  CPU only."""
import ctypes as C

import numpy as np
import pytest

import aar
import live_gate_cases as gc
import live_gate_restated as gr


def test_defaults_and_struct_sizes():
    p = aar.tracker_gate_params()
    assert (p.k_median, p.min_px, p.min_detections) == (6.0, 3.0, 4)
    assert p.struct_size == C.sizeof(aar.CTrackerGateParams) == 32
    assert C.sizeof(aar.CTrackerGateInfo) == 48
    assert aar.CTrackerGateParams.min_detections.offset == 24 and aar.CTrackerGateInfo.median.offset == 24
    aar.tracker_gate_params_validate()
    aar.tracker_gate_params_validate(k_median=0.0, min_px=2.0)          # a fixed threshold
    aar.tracker_gate_params_validate(k_median=3.0, min_px=0.0)          # the median alone
    aar.tracker_gate_params_validate(min_detections=1)
    aar.tracker_gate_params_validate(struct_size=28)                    # just reaches min_detections
    aar.tracker_gate_params_validate(struct_size=64)                    # a longer (newer) struct: the known fields are read


@pytest.mark.parametrize("kw,field", [
    (dict(struct_size=27), "struct_size"), (dict(struct_size=8), "struct_size"),
    (dict(min_px=float("nan")), "min_px"), (dict(min_px=float("inf")), "min_px"), (dict(min_px=-1.0), "min_px"),
    (dict(k_median=float("nan")), "k_median"), (dict(k_median=float("inf")), "k_median"),
    (dict(k_median=0.0, min_px=0.0), "both"), (dict(k_median=-2.0, min_px=0.0), "both"),
    (dict(min_detections=0), "min_detections"), (dict(min_detections=-3), "min_detections")])
def test_validate_refuses_and_names_the_field(kw, field):
    with pytest.raises(aar.AarError) as e:
        aar.tracker_gate_params_validate(**kw)
    assert e.value.code == aar.AAR_ERR_INVALID
    msg = str(e.value)
    assert "aar_tracker_gate_params" in msg and field in msg
    if field == "both":
        assert "k_median" in msg and "min_px" in msg


def test_null_arguments_are_refused_without_a_device():
    L = aar.lib()
    assert L.aar_tracker_gate_params_validate(None) == aar.AAR_ERR_INVALID
    assert L.aar_tracker_enable_gate(None, None) == aar.AAR_ERR_INVALID
    assert L.aar_tracker_gate_bank_enable(None, None) == aar.AAR_ERR_INVALID
    bad = aar.tracker_gate_params(min_px=-1.0)                          # the parameters are checked before the handle
    assert L.aar_tracker_enable_gate(None, C.byref(bad)) == aar.AAR_ERR_INVALID and "min_px" in L.aar_last_error().decode()
    g = aar.CTrackerGateInfo()
    assert L.aar_tracker_last_gate(None, C.byref(g)) == aar.AAR_ERR_INVALID
    assert L.aar_tracker_gate_detail(None, None, None, None) == aar.AAR_ERR_INVALID
    assert L.aar_tracker_gate_bank_last(None, 0, C.byref(g)) == aar.AAR_ERR_INVALID
    assert L.aar_tracker_gate_bank_detail(None, 0, None, None, None) == aar.AAR_ERR_INVALID


# ---- the restated rule on hand-worked lists ----
def test_lower_median_of_even_and_odd_n():
    g = gr.rule([4.0, 1.0, 3.0, 2.0], 2.0, 0.5, 4)                      # ascending 1 2 3 4: element floor(3/2) = 1 -> 2
    assert (g["median"], g["max"], g["threshold"], g["gated"]) == (2.0, 4.0, 4.0, 1) and list(g["keep"]) == [True, True, True, True]
    g = gr.rule([4.0, 1.0, 3.0, 2.0, 9.0], 2.0, 0.5, 4)                 # ascending 1 2 3 4 9: element 2 -> 3
    assert (g["median"], g["max"], g["threshold"]) == (3.0, 9.0, 6.0) and list(g["keep"]) == [True, True, True, True, False]
    assert (g["n_in"], g["n_kept"], g["n_nonfinite"]) == (5, 4, 0)
    g = gr.rule([1.0, 1.0, 1.0, 100.0], 6.0, 7.0, 4)                    # min_px wins over k * median = 6
    assert g["threshold"] == 7.0 and g["n_kept"] == 3
    g = gr.rule([5.0, 5.0, 5.0, 30.0], 6.0, 3.0, 4)                     # e_d == t is kept
    assert g["threshold"] == 30.0 and g["n_kept"] == 4


def test_non_finite_sorts_last_and_is_rejected():
    g = gr.rule([2.0, np.nan, 1.0, np.inf, 3.0, 1.5], 100.0, 0.0, 4)    # ascending 1 1.5 2 3 inf inf: element 2 -> 2
    assert (g["median"], g["max"], g["n_nonfinite"], g["n_kept"]) == (2.0, np.inf, 2, 4)
    assert list(g["keep"]) == [True, False, True, False, True, True]
    g = gr.rule([np.nan, np.nan, np.nan, 1.0], 6.0, 3.0, 4)             # the median itself is non-finite: t = +inf, and still none of them is kept
    assert g["median"] == np.inf and g["threshold"] == np.inf and list(g["keep"]) == [False, False, False, True]


def test_k_median_not_positive_and_small_frames():
    for k in (0.0, -1.0):
        g = gr.rule([1.0, 2.0, 3.0, 4.0], k, 2.5, 4)
        assert g["threshold"] == 2.5 and list(g["keep"]) == [True, True, False, False]
    g = gr.rule([1.0, 200.0, np.nan], 6.0, 3.0, 4)                      # fewer than min_detections: not gated, everything kept
    assert (g["gated"], g["n_kept"], g["threshold"], g["n_nonfinite"]) == (0, 3, np.inf, 1) and all(g["keep"])
    g = gr.rule([], 6.0, 3.0, 4)
    assert (g["gated"], g["n_in"], g["n_kept"], g["median"], g["max"], g["threshold"]) == (0, 0, 0, 0.0, 0.0, np.inf)
    g = gr.rule([1.0, 200.0, 2.0], 6.0, 3.0, 3)
    assert g["gated"] == 1 and list(g["keep"]) == [True, False, True]


def test_e_d_is_the_rms_corner_distance():
    c = gc.frames()["even-truth"]
    r = gc.gr.tr.residuals(c.fd, c.z0)
    want = [np.sqrt(sum(r[d, k, 0] ** 2 + r[d, k, 1] ** 2 for k in range(4)) / 4) for d in range(len(c.cam))]
    np.testing.assert_allclose(c.e, want, rtol=1e-14)
    e, med, mx, thr, keep = gr.gate(c.fd, c.z0, **c.rule)
    assert np.array_equal(e, c.e) and (med, mx, thr) == (c.g["median"], c.g["max"], c.g["threshold"]) and np.array_equal(keep, c.g["keep"])


# ---- the cases ----
def test_every_case_holds_the_margin_condition():
    fr = gc.frames()
    assert len(fr) == 15
    for name, c in fr.items():
        assert gc.margin(c.e, c.g), name
    sizes = {len(c.cam) for c in fr.values()}
    assert {3, 4, 300, 4096} <= sizes and any(n % 2 for n in sizes - {3}) and any(n % 2 == 0 for n in sizes - {4, 300, 4096})
    for start in ("truth", "pert"):
        assert fr["n3-" + start].g["gated"] == 0 and fr["n3-" + start].g["n_kept"] == 3
        assert fr["n4-" + start].g["gated"] == 1
        t = fr["ties-" + start]
        key = np.sort(t.e)
        m = (len(key) - 1) // 2
        assert key[m] == key[m - 1] or key[m] == key[m + 1]                              # a tie at the median position
        big = fr["n300-" + start]
        assert big.bad[:10].sum() >= 3 and (~big.g["keep"][:10]).sum() >= 1 and (~big.g["keep"][256:]).sum() >= 1
    for name in ("n4-pert", "odd-pert", "even-pert", "n300-pert"):                       # k_median * median decides, not min_px
        assert fr[name].g["threshold"] > 5 * gc.DEFAULT["min_px"], name
    for name in ("n4-truth", "odd-truth", "even-truth", "n300-truth", "n4096-odd"):      # at the truth the planted outliers are exactly the rejected
        assert np.array_equal(~fr[name].g["keep"], fr[name].bad), name
    odd = fr["n4096-odd"]
    assert np.array_equal(odd.g["keep"], np.arange(4096) % 2 == 0)
    assert fr["nonfinite"].g["n_nonfinite"] == 2 and fr["empty"].g["n_kept"] == 0


def test_the_streams_margins_at_the_perturbed_truth():
    c = gc.scene()
    planted = 0
    for f, (cam, mk, uv, bad) in enumerate(gc.stream()):
        fd = gc.ld.frame_data(c, cam, mk, uv)
        for z0 in (gc.truth(f), gc.perturbed(f)):
            e = gr.det_err(fd, z0)
            assert gc.margin(e, gr.rule(e, **gc.DEFAULT)), f
        g = gr.rule(gr.det_err(fd, gc.truth(f)), **gc.DEFAULT)
        if g["gated"]:
            assert np.array_equal(~g["keep"], bad), f
            planted += int(bad.sum())
        else:
            assert len(cam) == 3 and bad.sum() == 1 and g["n_kept"] == 3
    assert planted == sum(len(v) for k, v in gc.PLAN.items() if k not in gc.SHORT)
    assert np.all(np.diff(gc.TIMES) > 0)
