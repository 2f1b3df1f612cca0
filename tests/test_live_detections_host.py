"""Host side of the raw-detection live tracker (aar_tracker_enable_detections / aar_tracker_push_detections): the
parameter validation, the struct layouts, the refusal without a device, and the CPU yardstick of the GPU tests' scenes.  CPU only."""
import ctypes as C

import numpy as np
import pytest

import aar
import live_detection_cases as ld


def test_defaults_and_struct_sizes():
    p, _ = aar.tracker_detection_params()
    # the library writes its own sizeof into struct_size: the ctypes layout is the header's
    assert p.struct_size == C.sizeof(aar.CTrackerDetectionParams) == 32
    assert (p.ippe_threshold, p.min_detections, p.start_policy) == (2.0, 2, aar.TRACKER_START_VOTE) and not p.cams
    assert (aar.TRACKER_START_VOTE, aar.TRACKER_START_BEST) == (1, 2)
    assert C.sizeof(aar.CTrackerStartInfo) == 96 and aar.CTrackerStartInfo.start_pose.offset == 48 and aar.CTrackerStartInfo.vote_cost.offset == 16
    lib = C.CDLL(aar.LIB_PATH)
    for n in ("aar_tracker_default_detection_params", "aar_tracker_detection_params_validate", "aar_tracker_enable_detections",
              "aar_tracker_push_detections"):
        assert hasattr(lib, n) and n in aar.SYMBOLS, n


def test_validation_names_the_field():
    c = ld.case(False)
    aar.tracker_detection_params_validate(c.sol)
    aar.tracker_detection_params_validate(c.sol, Ks=c.K, dists=ld.case(True).dists, ippe_threshold=1e9, min_detections=1, start_policy="best")
    badK = np.array(c.K)
    badK[2, 1, 1] = np.inf
    cases = [(dict(struct_size=16), "struct_size"), (dict(struct_size=28), "struct_size"),
             (dict(ippe_threshold=0.0), "ippe_threshold"), (dict(ippe_threshold=-1.0), "ippe_threshold"), (dict(ippe_threshold=np.inf), "ippe_threshold"),
             (dict(ippe_threshold=np.nan), "ippe_threshold"), (dict(min_detections=0), "min_detections"), (dict(start_policy=0), "start_policy"),
             (dict(start_policy=3), "start_policy"), (dict(Ks=badK, dists=c.dists), "cams[2].K[4]")]
    for kw, word in cases:
        with pytest.raises(aar.AarError) as e:
            aar.tracker_detection_params_validate(c.sol, **kw)
        assert e.value.code == aar.AAR_ERR_INVALID and word in str(e.value), (kw, str(e.value))


def test_enable_detections_needs_a_device():
    if aar.device_count() > 0:
        pytest.skip("GPU present")
    p, _ = aar.tracker_detection_params()
    rc = aar.lib().aar_tracker_enable_detections(None, C.byref(p))     # (no tracker can exist without a device)
    assert rc == aar.AAR_ERR_NO_DEVICE


@pytest.mark.parametrize("distorted", [False, True], ids=["nodist", "dist8"])
def test_the_scenes_are_valid_for_the_gpu_tests(distorted):
    c = ld.case(distorted)
    ids, T, z = ld.oracle_object_poses(distorted)
    # one object pose per frame, every winner finite, and near the truth (0.2 px noise)
    assert list(ids) == list(c.ds.frame_ids) and len(T) == ld.FRAMES and np.all(np.isfinite(T))
    assert np.abs(T - c.fr).max() < 0.05
    cnt = [len(f[0]) for f in c.frames]
    assert min(cnt) >= 6 and all(len(np.unique(f[0])) >= 3 for f in c.frames)
    # the helpers: projecting the truth reproduces the detections up to the noise
    cam, mk, uv = c.frames[3]
    if not distorted:
        zt = c.ds.x_truth[c.ns + 18:c.ns + 24]
        assert np.abs(ld.project(c, cam, mk, zt) - uv).max() < 1.5
    rc, rm, ruv = ld.root_only_detection(c, 2)
    assert np.all(rc == c.ds.root_cam) and np.all(rm == c.ds.root_marker) and np.all((ruv > 0) & (ruv < 1280))
