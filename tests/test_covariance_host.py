"""aar_problem_covariance / aar_covariance_write_yaml without a GPU: the entry points exist, the compute call refuses to run
without a device, and the YAML writer round-trips (NaN blocks as `.nan`).  CPU only."""
import ctypes as C
import re

import numpy as np
import pytest

import aar
from conftest import load_golden


def test_covariance_entry_points_are_exported():
    lib = C.CDLL(aar.LIB_PATH)
    for n in ("aar_problem_covariance", "aar_covariance_write_yaml"):
        assert hasattr(lib, n) and n in aar.SYMBOLS
    assert hasattr(aar.Problem, "covariance")
    assert C.sizeof(aar.CCovarianceReport) == 64


@pytest.mark.skipif(aar.device_count() > 0, reason="this check is for machines without a GPU")
def test_covariance_without_a_device_is_no_device():
    rep = aar.CCovarianceReport()
    rep.struct_size = C.sizeof(rep)
    x = np.zeros(8)
    # no problem can exist without a device: the creation refuses, as for every other compute call
    ds, _ = load_golden("g2_small")
    with pytest.raises(aar.AarError) as e:
        aar.Problem(ds)
    assert e.value.code == aar.AAR_ERR_NO_DEVICE
    # ... and a null problem is an invalid argument, not a crash
    rc = aar.lib().aar_problem_covariance(None, x.ctypes.data_as(C.POINTER(C.c_double)), None, None, None, C.byref(rep))
    assert rc == aar.AAR_ERR_INVALID


def parse_cov_yaml(path):
    """A small parser of the writer's dialect: {section: {id: (sigma_rot, sigma_trans, 6x6)}} and sigma2."""
    txt = open(path).read()
    assert txt.startswith("%YAML:1.0\n---\n")
    num = lambda s: float(s.replace(".nan", "nan").replace(".inf", "inf"))
    out = {"sigma2": num(re.search(r"^sigma2: (\S+)$", txt, re.M).group(1))}
    for sec in re.finditer(r"^(\w+):\n((?:   - .*\n(?:       .*\n)*)*)", txt, re.M):
        recs = {}
        for m in re.finditer(r"- \{ (\w+):(-?\d+), sigma_rot: (\S+), sigma_trans: (\S+),\s*covariance: !!opencv-matrix \{ rows:6, cols:6, dt:d, data:\[([^\]]*)\] \} \}",
                             sec.group(2)):
            vals = np.array([num(v) for v in m.group(5).replace("\n", " ").split(",")])
            recs[int(m.group(2))] = (num(m.group(3)), num(m.group(4)), vals.reshape(6, 6))
        out[sec.group(1)] = recs
    return out


def test_covariance_yaml_round_trip(tmp_path):
    ds, _ = load_golden("g2_small")
    C_, M_ = ds.num_cams, ds.num_markers
    rng = np.random.default_rng(3)
    blocks = []
    for _ in range(C_ - 1 + M_ - 1):
        a = rng.normal(size=(6, 6))
        blocks.append(a @ a.T + 6 * np.eye(6))
    blocks[0][2, :] = np.nan     # an unobserved-style block
    blocks[0][:, 2] = np.nan
    diag = np.concatenate([b.reshape(-1) for b in blocks])
    frames = np.stack([np.eye(6) * (f + 1) for f in range(ds.num_frames)])
    frames[1] = np.nan
    sigma2 = 0.09
    path = str(tmp_path / "c.yaml")
    aar.covariance_write_yaml(path, ds, diag, sigma2, frames)
    txt = open(path).read()
    assert ".nan" in txt and "nan," not in txt.replace(".nan", "")
    y = parse_cov_yaml(path)
    assert y["sigma2"] == sigma2
    assert set(y["cameras"]) == set(int(i) for i in ds.cam_ids)
    assert set(y["markers"]) == set(int(i) for i in ds.marker_ids)
    assert len(y["object_poses"]) == ds.num_frames
    rc, rm = ds.root_cam, ds.root_marker
    k = 0
    for c in range(C_):
        sr, st, blk = y["cameras"][int(ds.cam_ids[c])]
        if c == rc:
            assert np.isnan(blk).all() and np.isnan(sr) and np.isnan(st)   # the root has no unknowns
            continue
        want = sigma2 * blocks[k]
        np.testing.assert_array_equal(np.isnan(blk), np.isnan(want))
        np.testing.assert_allclose(blk[~np.isnan(blk)], want[~np.isnan(want)], rtol=1e-15)
        if k > 0:
            np.testing.assert_allclose(sr, np.sqrt(np.trace(want[:3, :3]) / 3), rtol=1e-15)
            np.testing.assert_allclose(st, np.sqrt(np.trace(want[3:, 3:]) / 3), rtol=1e-15)
        k += 1
    for m in range(M_):
        sr, st, blk = y["markers"][int(ds.marker_ids[m])]
        if m == rm:
            assert np.isnan(blk).all()
            continue
        np.testing.assert_allclose(blk, sigma2 * blocks[k], rtol=1e-15)
        k += 1
    fids = [int(i) for i in ds.frame_ids]
    assert np.isnan(y["object_poses"][fids[1]][2]).all()
    np.testing.assert_allclose(y["object_poses"][fids[2]][2], sigma2 * 3 * np.eye(6), rtol=1e-15)


def test_covariance_yaml_without_frames_and_bad_path(tmp_path):
    ds, _ = load_golden("g2_small")
    diag = np.tile(np.eye(6).reshape(-1), ds.num_cams - 1 + ds.num_markers - 1)
    path = str(tmp_path / "c.yaml")
    aar.covariance_write_yaml(path, ds, diag, 1.0)
    y = parse_cov_yaml(path)
    assert "object_poses" not in y and len(y["markers"]) == ds.num_markers
    with pytest.raises(aar.AarError) as e:
        aar.covariance_write_yaml(str(tmp_path / "no" / "such" / "dir.yaml"), ds, diag, 1.0)
    assert e.value.code == aar.AAR_ERR_IO
