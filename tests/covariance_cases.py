"""The cases of the covariance certificates (tests/test_covariance_certificate_host.py, tests/test_gpu_covariance_certificates.py), by name --
TEST INFRASTRUCTURE ONLY.  CASES maps a name to (data-set builder, keywords); case_keywords turns the keywords into what aar.Problem and the
oracle take."""
import numpy as np

import aar
import direct_cases as dc
from conftest import load_golden
from reduced_system import slot_col


def x0_of(ds, intrinsics):
    x = np.asarray(ds.x_full, dtype=np.float64)
    if not intrinsics:
        return x
    K = np.asarray(ds.cam_mats, dtype=np.float64).reshape(-1, 9)
    d = np.asarray(ds.dist_coeffs, dtype=np.float64).reshape(-1, 5)
    return np.concatenate([x, np.concatenate([np.stack([K[:, 0], K[:, 2], K[:, 4], K[:, 5]], axis=1), d], axis=1).reshape(-1)])


def fixed_of(ds):
    fc = [c for c in range(ds.num_cams) if c != ds.root_cam][:2]
    fm = [m for m in range(ds.num_markers) if m != ds.root_marker][3:4]
    return dict(fixed_cams=fc, fixed_markers=fm)


def priors_of(ds, x, skip=()):
    """a prior on every camera that is neither the root nor in `skip`"""
    rng = np.random.default_rng(3)
    pr = []
    for c in range(ds.num_cams):
        if c != ds.root_cam and c not in skip:
            col = slot_col(ds, "camera", c)
            A = rng.standard_normal((6, 6))
            pr.append(("camera", c, x[col:col + 6] + np.r_[0.02 * rng.standard_normal(3), 0.01 * rng.standard_normal(3)], 1e3 * (A @ A.T + 6 * np.eye(6))))
    return pr


# name -> (data set, Problem / Oracle keywords; fixed="auto": fixed_of(ds); priors=True: priors_of on every camera that is not fixed)
CASES = {}
for _nT in range(1, 15):
    CASES["sweep%d" % _nT] = (lambda nT=_nT: dc.sweep_ds(nT), {})
for _c in (15, 16, 34):
    CASES["gauge_c%d" % _c] = (lambda c=_c: dc.gauge_ds(c, 3), {})
for _t in (3, 5):
    CASES["cams_off_%d" % _t] = (lambda t=_t: dc.gauge_ds(16, t), dict(optimize=(False, True, True)))
    CASES["markers_off_%d" % _t] = (lambda t=_t: dc.gauge_ds(16, t), dict(optimize=(True, False, True)))
    CASES["fixed_%d" % _t] = (lambda t=_t: dc.gauge_ds(16, t), dict(fixed="auto"))
CASES["worklist_unseen"] = (lambda: dc.without_pairs(dc.worklist_ds(60), 7, 11), {})
CASES["empty_frame"] = (lambda: dc.without_frame(dc.sweep_ds(2), 5), {})
CASES["roots_only_frame"] = (lambda: dc.roots_only_frame(dc.worklist_ds(60))[0], {})
CASES["small_frames"] = (dc.small_frames_ds, {})
# (no frame of the intrinsics fixture can be cut to 11 slots: three of its frames are cut to 3, 6 and 10, beside its own of 12 and 13; the synthetic
# set with intrinsics entities is cut to all five)
CASES["small_frames_intr_fixture"] = (lambda: dc.cut_frames(load_golden("g1_cfg2_intr")[0], dc.SMALL_TARGETS_INTRINSICS[:3], True)[0], dict(intrinsics=True))
CASES["small_frames_intr"] = (lambda: dc.cut_frames(aar.synth(2, num_cams=4, num_markers=12, num_frames=16, min_view_cos=0.01, seed=800),
                                                    dc.SMALL_TARGETS_INTRINSICS, True)[0], dict(intrinsics=True))
for _m in (84, 92):
    CASES["wide_%d" % _m] = (lambda m=_m: dc.wide_frames_ds(m), {})
CASES["huber"] = (lambda: load_golden("g1_cfg2_huber")[0], dict(with_huber=True))
CASES["intrinsics"] = (lambda: load_golden("g1_cfg2_intr")[0], dict(intrinsics=True))
CASES["priors_fixed"] = (lambda: load_golden("g1_cfg3_cut")[0], dict(fixed="one", priors=True))
CASES["g2_small"] = (lambda: load_golden("g2_small")[0], {})
CASES["cfg3"] = (lambda: aar.synth(3), {})
CASES["cfg5_shaped"] = (lambda: aar.synth(5, num_frames=40), {})
# (sets of the conditioning table that the device module reaches through other families)
CASES["mfma_F1"] = (lambda: dc.mfma_frames_ds(1), {})
CASES["worklist_F3"] = (lambda: dc.worklist_ds(3), {})
CASES["dense_32"] = (lambda: dc.dense_count_ds(32), {})


def case_keywords(ds, kw, x):
    """(optimize, intrinsics, with_huber, fixed dict, priors list) of a case"""
    fixed = {}
    if kw.get("fixed") == "auto":
        fixed = fixed_of(ds)
    elif kw.get("fixed") == "one":
        fixed = dict(fixed_cams=[c for c in range(ds.num_cams) if c != ds.root_cam][:1], fixed_markers=[])
    pri = priors_of(ds, x, skip=fixed.get("fixed_cams", ())) if kw.get("priors") else []
    return kw.get("optimize", (True, True, True)), kw.get("intrinsics", False), kw.get("with_huber", False), fixed, pri
