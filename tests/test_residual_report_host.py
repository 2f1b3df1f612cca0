"""aar_problem_residual_report / aar_dataset_select_observations / aar_residual_report_write_yaml without a GPU: the entry points exist,
the compute call refuses bad arguments without crashing, observation selection keeps what it must, and the YAML writer round-trips.
CPU only."""
import ctypes as C
import re

import numpy as np
import pytest

import aar
from conftest import load_golden


def test_residual_report_entry_points_are_exported():
    lib = C.CDLL(aar.LIB_PATH)
    for n in ("aar_problem_residual_report", "aar_dataset_select_observations", "aar_residual_report_write_yaml"):
        assert hasattr(lib, n) and n in aar.SYMBOLS
    assert hasattr(aar.Problem, "residual_report") and hasattr(aar.Dataset, "select_observations")
    # the C layouts (include/aar.h): uint32 + pad, 2 doubles | uint32 + pad, 3 int64, 5 doubles, 3 int32 + pad
    assert C.sizeof(aar.COutlierRule) == 24
    assert C.sizeof(aar.CResidualReport) == 88
    assert aar.CResidualReport.threshold.offset == 64 and aar.CResidualReport.frames_emptied.offset == 80


def _report_args():
    rep = aar.CResidualReport()
    rep.struct_size = C.sizeof(rep)
    x = np.zeros(8)
    return rep, x, x.ctypes.data_as(C.POINTER(C.c_double))


def test_report_call_refuses_bad_arguments_without_a_crash():
    rep, _, xp = _report_args()
    L = aar.lib()
    assert L.aar_problem_residual_report(None, xp, None, None, None, None, None, None, C.byref(rep)) == aar.AAR_ERR_INVALID
    assert L.aar_problem_residual_report(None, xp, None, None, None, None, None, None, None) == aar.AAR_ERR_INVALID
    assert "null argument" in L.aar_last_error().decode()


@pytest.mark.skipif(aar.device_count() > 0, reason="this check is for machines without a GPU")
def test_report_without_a_device_is_no_device():
    ds, _ = load_golden("g2_small")
    with pytest.raises(aar.AarError) as e:
        aar.Problem(ds)   # no problem can exist without a device, so neither can its report
    assert e.value.code == aar.AAR_ERR_NO_DEVICE


def _same(a, b):
    for f in aar.Dataset.FIELDS:
        va, vb = getattr(a, f), getattr(b, f)
        if va is None or vb is None:
            assert va is None and vb is None, f
        else:
            assert np.array_equal(va, vb), f
    for f in ("num_cams", "num_markers", "num_frames", "root_cam", "root_marker", "marker_size", "num_obs", "optimize_cam_poses",
              "optimize_marker_poses", "optimize_object_poses", "optimize_cam_intrinsics"):
        assert getattr(a, f) == getattr(b, f), f


def test_select_all_ones_is_the_same_data_set():
    ds = aar.synth(2)
    assert ds.x_truth is not None
    _same(ds.select_observations(np.ones(ds.num_obs, dtype=bool)), ds)


def test_select_keeps_order_and_empty_frames():
    ds, _ = load_golden("g1_cfg2")
    rng = np.random.default_rng(5)
    keep = rng.random(ds.num_obs) > 0.3
    keep[ds.obs_frame == 4] = False            # frame 4 loses every detection
    keep[ds.obs_marker == 1] = False           # ... and marker 1
    out = ds.select_observations(keep)
    assert out.num_obs == keep.sum()
    assert out.num_frames == ds.num_frames and out.num_markers == ds.num_markers and out.num_cams == ds.num_cams
    for f in ("obs_frame", "obs_cam", "obs_marker", "obs_uv"):
        assert np.array_equal(getattr(out, f), getattr(ds, f)[keep]), f
    assert (np.diff(out.obs_frame) >= 0).all()
    assert 4 not in set(out.obs_frame.tolist()) and 1 not in set(out.obs_marker.tolist())
    for f in ("cam_ids", "marker_ids", "frame_ids", "cam_mats", "dist_coeffs", "image_sizes", "x_full"):
        assert np.array_equal(getattr(out, f), getattr(ds, f)), f


def test_select_refuses_wrong_length_and_null():
    ds, _ = load_golden("g2_small")
    with pytest.raises(ValueError):
        ds.select_observations(np.ones(ds.num_obs - 1, dtype=bool))
    c = ds.as_c()
    out = C.POINTER(aar.CDataset)()
    assert aar.lib().aar_dataset_select_observations(C.byref(c), None, C.byref(out)) == aar.AAR_ERR_INVALID
    k = np.ones(ds.num_obs, dtype=np.uint8)
    assert aar.lib().aar_dataset_select_observations(None, k.ctypes.data_as(C.POINTER(C.c_uint8)), C.byref(out)) == aar.AAR_ERR_INVALID


def parse_residual_yaml(path):
    """A small parser of the writer's dialect: scalars, {section: {id: dict}} and the list of rejected detections."""
    txt = open(path).read()
    assert txt.startswith("%YAML:1.0\n---\n")
    num = lambda s: float(s.replace(".nan", "nan").replace(".inf", "inf"))
    out = {m.group(1): num(m.group(2)) for m in re.finditer(r"^(\w+): (\S+)$", txt, re.M)}
    for sec, key in (("cameras", "cam_id"), ("markers", "marker_id")):
        body = re.search(r"^%s:\n((?:   - .*\n)*)" % sec, txt, re.M).group(1)
        recs = {}
        for m in re.finditer(r"- \{ %s:(-?\d+), detections:(\d+), rmse: (\S+), max: (\S+), rejected:(\d+) \}" % key, body):
            recs[int(m.group(1))] = dict(detections=int(m.group(2)), rmse=num(m.group(3)), max=num(m.group(4)), rejected=int(m.group(5)))
        out[sec] = recs
    m = re.search(r"^rejected_detections:\n((?:   - .*\n)*)", txt, re.M)
    out["rejected_detections"] = None if m is None else [
        (int(a), int(b), int(c), num(e)) for a, b, c, e in
        re.findall(r"- \{ frame_id:(-?\d+), cam_id:(-?\d+), marker_id:(-?\d+), error: (\S+) \}", m.group(1))]
    return out


def _fake_report(ds, rng):
    e = rng.random(ds.num_obs) + 0.1
    e[3] = np.nan
    keep = e <= 0.9
    cs = np.zeros((ds.num_cams, 4))
    ms = np.zeros((ds.num_markers, 4))
    for st, idx, n in ((cs, ds.obs_cam, ds.num_cams), (ms, ds.obs_marker, ds.num_markers)):
        for i in range(n):
            sel = idx == i
            if sel.any():
                st[i] = (sel.sum(), (4 * e[sel] ** 2).sum(), np.max(e[sel]), (~keep[sel]).sum())
    rep = dict(num_detections=ds.num_obs, num_rejected=int((~keep).sum()), num_nonfinite=1, sum_sq=float(np.nansum(4 * e ** 2)), rmse=0.5,
               median=float(np.sort(e)[(ds.num_obs - 1) // 2]), max=float("nan"), threshold=0.9, cams_emptied=0, markers_emptied=1, frames_emptied=2)
    return aar.ResidualReport(det_err=e, keep=keep, cam_stats=cs, marker_stats=ms, frame_stats=None, report=rep)


def test_residual_yaml_round_trip(tmp_path):
    ds, _ = load_golden("g1_cfg2")
    rr = _fake_report(ds, np.random.default_rng(7))
    path = str(tmp_path / "r.yaml")
    aar.residual_report_write_yaml(path, ds, rr)
    y = parse_residual_yaml(path)
    for k, v in rr.report.items():
        if isinstance(v, float) and np.isnan(v):
            assert np.isnan(y[k]), k
        else:
            assert y[k] == v, k
    for sec, st, ids in (("cameras", rr.cam_stats, ds.cam_ids), ("markers", rr.marker_stats, ds.marker_ids)):
        assert set(y[sec]) == set(int(i) for i in ids)
        for i, id_ in enumerate(ids):
            r = y[sec][int(id_)]
            assert r["detections"] == st[i, 0] and r["rejected"] == st[i, 3]
            if st[i, 0] > 0:
                np.testing.assert_allclose(r["rmse"], np.sqrt(st[i, 1] / (4 * st[i, 0])), rtol=1e-15)
            assert r["max"] == st[i, 2] or (np.isnan(r["max"]) and np.isnan(st[i, 2]))
    want = [(int(ds.frame_ids[ds.obs_frame[o]]), int(ds.cam_ids[ds.obs_cam[o]]), int(ds.marker_ids[ds.obs_marker[o]]), rr.det_err[o])
            for o in np.flatnonzero(~rr.keep)]
    got = y["rejected_detections"]
    assert len(got) == len(want) > 0
    for g, w in zip(got, want):
        assert g[:3] == w[:3] and (g[3] == w[3] or (np.isnan(g[3]) and np.isnan(w[3])))
    # without the per-detection arrays: no list; a directory that does not exist: an I/O error
    aar.residual_report_write_yaml(path, ds, rr, det_err=False)
    assert parse_residual_yaml(path)["rejected_detections"] is None
    with pytest.raises(aar.AarError) as e:
        aar.residual_report_write_yaml(str(tmp_path / "no" / "such" / "dir.yaml"), ds, rr)
    assert e.value.code == aar.AAR_ERR_IO
