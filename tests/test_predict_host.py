"""The host surface of the predicted corners and detection leverages (include/aar.h): the query validation, the exported
symbols, the refusal without a device and the YAML writer.  CPU only."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import aar
from conftest import PKG, ROOT, load_golden

NEW = ["aar_predict_query_validate", "aar_problem_predict_corners", "aar_problem_detection_leverage", "aar_leverage_write_yaml"]


def _ds():
    return load_golden("g2_small")[0]


def test_symbols_are_exported_and_listed():
    lib = C.CDLL(aar.LIB_PATH)
    for n in NEW:
        assert hasattr(lib, n), n
        assert n in aar.SYMBOLS
    assert C.sizeof(aar.CPredictReport) == 88      # (the struct of include/aar.h: eleven 8-byte slots)
    assert (aar.PREDICT_BEHIND, aar.PREDICT_UNDEFINED) == (1, 2)


def test_query_validate_accepts_the_range_and_the_empty_set():
    ds = _ds()
    C_, M, F = ds.num_cams, ds.num_markers, ds.num_frames
    aar.predict_query_validate(ds, np.zeros((0, 3)))
    aar.predict_query_validate(ds, [[0, 0, 0], [C_ - 1, M - 1, F - 1], [0, 0, 0]])      # (duplicates are allowed)
    # n_query = 0 needs no arrays; a positive count does
    cds = ds.as_c()
    d = aar.CProblemDesc()
    aar.lib().aar_problem_desc_from_dataset(C.byref(cds), C.byref(d))
    assert aar.lib().aar_predict_query_validate(C.byref(d), 0, None, None, None) == aar.AAR_OK
    assert aar.lib().aar_predict_query_validate(C.byref(d), 1, None, None, None) == aar.AAR_ERR_INVALID
    assert "null query array" in aar.lib().aar_last_error().decode()
    assert aar.lib().aar_predict_query_validate(C.byref(d), -1, None, None, None) == aar.AAR_ERR_INVALID
    assert aar.lib().aar_predict_query_validate(None, 0, None, None, None) == aar.AAR_ERR_INVALID


@pytest.mark.parametrize("col,name,count", [(0, "q_cam", "num_cams"), (1, "q_marker", "num_markers"), (2, "q_frame", "num_frames")])
@pytest.mark.parametrize("how", ["negative", "too_large"])
def test_query_validate_names_the_first_offender(col, name, count, how):
    ds = _ds()
    n = getattr(ds, count)
    q = np.zeros((6, 3), dtype=np.int64)
    bad = -1 if how == "negative" else n
    q[3, col] = bad
    q[5, col] = bad - 7 if how == "negative" else bad + 7        # a later offender is not the one named
    with pytest.raises(aar.AarError) as e:
        aar.predict_query_validate(ds, q)
    assert e.value.code == aar.AAR_ERR_INVALID
    assert "%s[3] = %d" % (name, bad) in str(e.value) and "%s - 1 = %d" % (count, n - 1) in str(e.value)


def test_query_validate_reports_the_earliest_query_across_kinds():
    ds = _ds()
    q = np.zeros((4, 3), dtype=np.int64)
    q[2, 2] = ds.num_frames
    q[3, 0] = ds.num_cams
    with pytest.raises(aar.AarError, match=r"q_frame\[2\]"):
        aar.predict_query_validate(ds, q)


@pytest.mark.skipif(aar.device_count() > 0, reason="this check is for machines without a GPU")
def test_compute_entries_need_a_device():
    ds = _ds()
    with pytest.raises(aar.AarError) as e:
        aar.Problem(ds)          # no problem can exist without a device ...
    assert e.value.code == aar.AAR_ERR_NO_DEVICE
    x = np.zeros(8)
    dp = x.ctypes.data_as(C.POINTER(C.c_double))
    # ... and the entries say so themselves when they are handed none
    assert aar.lib().aar_problem_predict_corners(None, dp, 0, None, None, None, None, None, None, None) == aar.AAR_ERR_NO_DEVICE
    assert aar.lib().aar_problem_detection_leverage(None, dp, None, None, None) == aar.AAR_ERR_NO_DEVICE
    assert "no CPU path" in aar.lib().aar_last_error().decode()


def parse_leverage_yaml(path):
    """dict(scalars, cameras {id: (n, mean, max)}, markers, listed [(frame id, cam id, marker id, leverage, error)])"""
    num = r"([-+.\w]+)"
    out = dict(cameras={}, markers={}, listed=[])
    sect = None
    lines = open(path).read().splitlines()
    assert lines[0] == "%YAML:1.0" and lines[1] == "---"
    val = lambda s: float("nan") if s == ".nan" else (float("inf") if s == ".inf" else float(s))
    for ln in lines[2:]:
        m = re.match(r"^(\w+):\s*(\S*)$", ln)
        if m and m.group(2):
            out[m.group(1)] = val(m.group(2))
            continue
        if m:
            sect = m.group(1)
            continue
        m = re.match(r"^   - \{ (cam_id|marker_id):(-?\d+), detections:(\d+), mean: %s, max: %s \}$" % (num, num), ln)
        if m:
            out["cameras" if m.group(1) == "cam_id" else "markers"][int(m.group(2))] = (int(m.group(3)), val(m.group(4)), val(m.group(5)))
            assert sect == ("cameras" if m.group(1) == "cam_id" else "markers")
            continue
        m = re.match(r"^   - \{ frame_id:(-?\d+), cam_id:(-?\d+), marker_id:(-?\d+), leverage: %s, error: %s \}$" % (num, num), ln)
        assert m and sect == "high_leverage_detections", ln
        out["listed"].append((int(m.group(1)), int(m.group(2)), int(m.group(3)), val(m.group(4)), val(m.group(5))))
    return out


def test_leverage_yaml_round_trip(tmp_path):
    ds = _ds()
    N = ds.num_obs
    rng = np.random.default_rng(5)
    lev = rng.uniform(0.1, 7.9, N)
    lev[3] = 8.0
    lev[7] = np.nan                       # (a non-finite leverage is listed and kept out of the statistics)
    err = rng.uniform(0.0, 3.0, N)
    rep = dict(num_residuals=8 * N, num_vars=150, sum_sq=12.5, sigma2=0.093, num_live_vars=150, leverage_sum=float(np.nansum(lev)), undefined=0,
               behind=0, launches=40, seconds=1e-3)
    path = str(tmp_path / "final.leverage.yaml")
    aar.leverage_write_yaml(path, ds, lev, rep, h_min=6.0, det_err=err)
    y = parse_leverage_yaml(path)
    assert y["num_live_vars"] == 150 and y["h_min"] == 6.0
    np.testing.assert_allclose([y["sigma2"], y["leverage_sum"]], [0.093, rep["leverage_sum"]], rtol=1e-6)
    fin = np.isfinite(lev)
    for key, ids, obs in (("cameras", ds.cam_ids, ds.obs_cam), ("markers", ds.marker_ids, ds.obs_marker)):
        assert set(y[key]) == set(int(i) for i in ids)
        for k, i in enumerate(ids):
            sel = (np.asarray(obs) == k) & fin
            n, mean, mx = y[key][int(i)]
            assert n == sel.sum()
            if n:
                np.testing.assert_allclose([mean, mx], [lev[sel].mean(), lev[sel].max()], rtol=1e-6)
            else:
                assert (mean, mx) == (0.0, 0.0)
    want = [o for o in range(N) if not lev[o] < 6.0]
    assert 3 in want and 7 in want and len(y["listed"]) == len(want)
    for row, o in zip(y["listed"], want):
        assert row[:3] == (int(ds.frame_ids[ds.obs_frame[o]]), int(ds.cam_ids[ds.obs_cam[o]]), int(ds.marker_ids[ds.obs_marker[o]]))
        if np.isnan(lev[o]):
            assert np.isnan(row[3])
        else:
            np.testing.assert_allclose(row[3], lev[o], rtol=1e-6)
        np.testing.assert_allclose(row[4], err[o], rtol=1e-6)
    # without det_err the errors are .nan; a NaN threshold and a missing report are refused
    aar.leverage_write_yaml(path, ds, lev, rep, h_min=7.5)
    y = parse_leverage_yaml(path)
    assert len(y["listed"]) == sum(1 for o in range(N) if not lev[o] < 7.5) and all(np.isnan(r[4]) for r in y["listed"])
    with pytest.raises(aar.AarError) as e:
        aar.leverage_write_yaml(path, ds, lev, rep, h_min=float("nan"))
    assert e.value.code == aar.AAR_ERR_INVALID
    c = ds.as_c()
    assert aar.lib().aar_leverage_write_yaml(path.encode(), C.byref(c), lev.ctypes.data_as(C.POINTER(C.c_double)), None, 1.0, None) == aar.AAR_ERR_INVALID
    with pytest.raises(aar.AarError) as e:
        aar.leverage_write_yaml(str(tmp_path / "no" / "dir.yaml"), ds, lev, rep)
    assert e.value.code == aar.AAR_ERR_IO


def build_mapper_tool(tmp_path):
    exe = str(tmp_path / "predict_mapper_main")
    cc = subprocess.run(["g++", "-O0", "-std=c++17", "-Wall", os.path.join(ROOT, "tests", "tools", "predict_mapper_main.cpp"), "-o", exe, "-L" + PKG, "-laar",
                         "-Wl,-rpath," + PKG, "-Wl,-rpath,/opt/rocm/lib"], capture_output=True, text=True)
    assert cc.returncode == 0, cc.stderr[-3000:]
    return exe


def test_mapper_maps_ids_and_names_an_unknown_one(tmp_path):
    # MultiCamMapper::predict_corners takes ids; an id the data set does not have is an error naming it, before any device is looked for
    run = subprocess.run([build_mapper_tool(tmp_path)], capture_output=True, text=True, timeout=120)
    kv = dict(ln.split(" = ", 1) for ln in run.stdout.splitlines() if " = " in ln)
    for what in ("camera", "marker", "frame"):
        assert re.fullmatch(r"MultiCamMapper: no %s with id \d+" % what, kv["unknown_" + what]), kv
    assert "differ in length" in kv["lengths"]
    if aar.device_count() == 0:
        assert run.returncode == 2 and "no CPU path" in kv["device"]
