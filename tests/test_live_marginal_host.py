"""The marginalised anchor and the per-push covariance of the live tracker on the host: the float64 restatement
tests/live_marginal_restated.py against numpy's elimination of the frame that left, against the batch smoother, and the host side of the
aar_tracker_* entry points (validation, size versioning, exported symbol).  CPU only."""
import ctypes as C
import functools

import numpy as np
import pytest

import aar
import live_marginal_cases as mc
import live_marginal_restated as lm
import pose_metrics as pm
import smooth_cases as sc
import smooth_restated as sr
import track_restated as tr

BATCH_LM = dict(min_avg=1e-12)     # both sides run to convergence: the stop rule must not be what is compared


# ---- 1. the marginal is the Schur complement of the frame that left ----
@pytest.mark.parametrize("lag", [1, 3, 15])
def test_marginal_is_the_schur_complement_of_the_frame_that_left(lag):
    c, ref = mc.case("counts", lag), mc.restated("counts", lag, "marginal")
    seen = 0
    for f in range(lag + 1, c.n):
        r, before = ref[f], ref[f - 1]
        if before["marginal"] is None:
            continue
        wp, z0, left = r["problem"], r["start"], r["left"]
        assert wp.prior is not None and np.array_equal(wp.prior[0], before["marginal"][0])
        d, o, b = wp.system(z0)
        # the window extended by the frame that just left, carrying the prior the PREVIOUS push used, at the same point
        ext = lm.WindowProblemM(c.td, [left[0]] + wp.frames, [left[1]] + [float(t) for t in c.times[wp.frames]], mc.SROT, mc.STRANS,
                                delta=-1.0 if c.delta is None else c.delta, prior=before["prior_in"])
        ze = np.vstack([left[2][None, :], z0])
        de, oe, be = ext.system(ze)
        H, He = sr.dense(d, o), sr.dense(de, oe)
        A, O = He[:6, :6], He[:6, 6:]
        S = He[6:, 6:] - O.T @ np.linalg.solve(A, O)
        g = be[6:] - O.T @ np.linalg.solve(A, be[:6])
        big = np.abs(He).max()
        assert np.abs(H - S).max() <= 1e-10 * big, (f, np.abs(H - S).max() / big)
        assert np.abs(b - g).max() <= 1e-10 * np.abs(be).max(), (f, np.abs(b - g).max() / np.abs(be).max())
        Hi, Hei = np.linalg.inv(H), np.linalg.inv(He)
        W = wp.F
        blk = np.stack([Hi[6 * i:6 * i + 6, 6 * i:6 * i + 6] for i in range(W)])
        blke = np.stack([Hei[6 * (i + 1):6 * (i + 1) + 6, 6 * (i + 1):6 * (i + 1) + 6] for i in range(W)])
        assert np.abs(blk - blke).max() <= 1e-10 * np.abs(Hei).max(), (f, np.abs(blk - blke).max() / np.abs(Hei).max())
        assert wp.rows == 8.0 * wp.detections + 6.0 * W          # W - 1 pairs and the prior
        seen += 1
    assert seen == c.n - lag - 1 and ref[-1]["dropped"] == 0


def test_restated_cases_drop_no_marginal():
    """what tests/test_gpu_live_marginal.py relies on: the restatement alone keeps every marginal in its cases"""
    for kind in ("counts", "huber", "far"):
        for lag in (1, 3, 15):
            ref = mc.restated(kind, lag, "marginal")
            assert ref[-1]["dropped"] == 0 and [r["has_marginal"] for r in ref] == [int(f >= lag) for f in range(len(ref))], (kind, lag)


def test_genuine_marginals_stay_far_above_the_drop_threshold():
    """The drop rule holds a pivot of L' against PIVOT_REL = 1e-10 of the pair's own diagonal entry of B.  L' = B - O^T A^-1 O is a difference
    of terms of the size of B, so its rounding noise is a few ulp of B (about 1e-16 B, measured 2e-17 at the empty start) and an L' below 1e-10 B
    keeps fewer than six digits: the threshold sits 1e6 above the noise.  What it must never catch is a real frame.  The smallest ratio over
    every kept marginal of the stream cases, and over the weakest real frame these scenes can make -- ONE detection, leaving through a prior
    2500 times tighter than the cases' (sigmas 1e-3 / 4e-4, the largest B against the least data) -- must stay at least 1e4 above it."""
    smallest = np.inf
    for kind in ("counts", "huber", "far"):
        for lag in (1, 3, 15):
            for r in mc.restated(kind, lag, "marginal"):
                if r["window_frames"] == lag + 1:
                    smallest = min(smallest, lm.pivot_ratios(r["problem"], r["z"]).min())
    print("smallest pivot ratio of a kept marginal in the stream cases: %.3e" % smallest)
    assert smallest > 1e4 * lm.PIVOT_REL
    c = mc.case("plain", 1)
    ds = mc.keep_first(c.ds, [1] + [None] * (c.n - 1))
    td = tr.TrackData(ds, c.x0)
    live = lm.LiveM(td, lag=1, smooth=True, sigma_rot=mc.SROT / 50, sigma_trans=mc.STRANS / 50, anchor="marginal")
    live.push(0, 0.0, pose_init=td.z0[0])
    r = live.push(1, 1.0, pose_init=td.z0[1])
    weak = lm.pivot_ratios(r["problem"], r["z"]).min()
    print("one detection behind a tight prior: smallest pivot ratio %.3e" % weak)
    assert r["has_marginal"] == 1 and r["dropped"] == 0 and weak > 1e4 * lm.PIVOT_REL


# ---- 2. a stream that starts with an empty frame ----
def test_empty_stream_start_drops_the_marginal_once():
    ref = mc.restated("plain", 3, "marginal", True, True)
    c = mc.case("plain", 3, True, True)
    assert np.bincount(c.ds.obs_frame, minlength=c.n)[0] == 0
    r = ref[3]                                              # the first full window: frame 0 leaves with neither prior nor detections
    Lp, bp, B = lm.marginal_terms(r["problem"], r["z"])
    print("empty start: |L'| / |B| = %.3e" % (np.abs(Lp).max() / np.abs(B).max()))
    assert np.abs(Lp).max() <= 1e-12 * np.abs(B).max()      # 0 up to rounding
    assert [x["dropped"] for x in ref] == [0, 0, 0] + [1] * (c.n - 3)
    assert [x["has_marginal"] for x in ref] == [0, 0, 0, 0] + [1] * (c.n - 4)
    assert ref[4]["problem"].prior is None and ref[4]["problem"].rows == 8.0 * ref[4]["problem"].detections + 6.0 * 3
    for x in ref:
        assert np.isfinite(x["z"]).all() and np.isfinite(x["err"]) and np.isfinite(x["cov"]).all()


# ---- 3. the batch property ----
@functools.lru_cache(maxsize=None)
def batch_distances():
    """{anchor: largest distance of a lagged pose to the batch smoother over the frames pushed so far}"""
    ds, x0 = mc.moving_object()
    n0, F, lag = sc.ns(ds), ds.num_frames, mc.BATCH_LAG
    td = tr.TrackData(ds, x0)

    def sub(n, z):
        keep = np.asarray(ds.obs_frame) <= n
        return sc.copy_of(ds, num_frames=n + 1, frame_ids=ds.frame_ids[:n + 1], obs_frame=ds.obs_frame[keep], obs_cam=ds.obs_cam[keep],
                          obs_marker=ds.obs_marker[keep], obs_uv=ds.obs_uv[keep], x_full=np.r_[x0[:n0], z.reshape(-1)])

    out, batch = {}, {}
    for anchor in ("fixed", "marginal"):
        live = lm.LiveM(td, lag=lag, smooth=True, sigma_rot=mc.BATCH_SROT, sigma_trans=mc.BATCH_STRANS, anchor=anchor, **BATCH_LM)
        hist, worst = np.zeros((F, 6)), 0.0
        for f in range(F):
            r = live.push(f, float(f), pose_init=td.z0[0] if f == 0 else None)
            w, _ = live.window()
            hist[f + 1 - len(w): f + 1] = w
            if r["lagged_pose"] is None:
                continue
            s = sub(f, hist[:f + 1])
            if f not in batch:
                sp = sr.SmoothProblem(tr.TrackData(s, s.x_full), mc.BATCH_SROT, mc.BATCH_STRANS, frame_time=np.arange(f + 1.0))
                batch[f] = sr.smooth_lm(sp, hist[:f + 1], **BATCH_LM)["z"]
            one = sc.copy_of(s, num_frames=1)
            worst = max(worst, max(pm.pose_delta(one, np.r_[x0[:n0], r["lagged_pose"]], np.r_[x0[:n0], batch[f][f - lag]])["frames"]))
        out[anchor] = worst
    return out


def test_marginal_anchor_is_closer_to_the_batch_smoother():
    d = batch_distances()
    print("batch property (restated, 24 frames, lag 3, sigmas %g / %g): fixed %.3e, marginal %.3e" % (
        mc.BATCH_SROT, mc.BATCH_STRANS, d["fixed"], d["marginal"]))
    assert d["marginal"] < d["fixed"]


# ---- 4. the host side of the C ABI ----
def test_params_validate_names_the_new_fields():
    ds = mc.case("counts", 3).ds
    good = dict(lag=3, smooth=True, sigma_rot=mc.SROT, sigma_trans=mc.STRANS)
    aar.tracker_params_validate(ds, anchor="marginal", covariance=True, **good)
    aar.tracker_params_validate(ds, lag=0, smooth=False, covariance=True)            # covariance alone, also without the prior
    aar.tracker_params_validate(ds, lag=0, smooth=True, sigma_rot=mc.SROT, sigma_trans=mc.STRANS, covariance=True)
    for kw, words in [(dict(good, anchor=2), ["anchor_mode"]), (dict(good, anchor=-1), ["anchor_mode"]),
                      (dict(lag=0, smooth=False, anchor="marginal"), ["anchor_mode", "smooth"]),
                      (dict(good, lag=0, anchor="marginal"), ["anchor_mode", "lag"]),
                      (dict(good, covariance=2), ["covariance"]), (dict(good, covariance=-1), ["covariance"])]:
        with pytest.raises(aar.AarError) as e:
            aar.tracker_params_validate(ds, **kw)
        assert e.value.code == aar.AAR_ERR_INVALID and all(w in str(e.value) for w in words), (kw, str(e.value))


def test_old_struct_size_means_fixed_anchor_and_no_covariance():
    ds = mc.case("counts", 3).ds
    old = aar.CTrackerParams.anchor_mode.offset
    assert old == aar.CTrackerParams.device_id.offset + 4 and C.sizeof(aar.CTrackerParams) == old + 8      # the two fields are appended
    # garbage behind the old end is not read
    aar.tracker_params_validate(ds, lag=3, smooth=True, sigma_rot=mc.SROT, sigma_trans=mc.STRANS, anchor=7, covariance=9, struct_size=old)
    aar.tracker_params_validate(ds, lag=0, smooth=False, anchor="marginal", struct_size=old)
    # ... and covariance alone is read when the struct ends behind anchor_mode
    with pytest.raises(aar.AarError) as e:
        aar.tracker_params_validate(ds, lag=3, smooth=True, sigma_rot=mc.SROT, sigma_trans=mc.STRANS, anchor=7, struct_size=old + 4)
    assert "anchor_mode" in str(e.value)
    p = aar.tracker_params()
    assert (p.anchor_mode, p.covariance) == (aar.TRACKER_ANCHOR_FIXED, 0) and aar.TRACKER_ANCHOR_MARGINAL == 1


def test_uncertainty_symbol_is_exported():
    lib = C.CDLL(aar.LIB_PATH)
    assert hasattr(lib, "aar_tracker_uncertainty") and "aar_tracker_uncertainty" in aar.SYMBOLS
    u = aar.CTrackerUncertainty
    assert u.cov.size == 16 * 36 * 8 and u.frame_index.size == 16 * 8 and u.marginal_info.size == 36 * 8
    with pytest.raises(aar.AarError) as e:                                            # validated before the device is touched
        aar.Tracker(mc.case("counts", 3).ds, lag=0, smooth=False, anchor="marginal")
    assert e.value.code == aar.AAR_ERR_INVALID and "anchor_mode" in str(e.value)
