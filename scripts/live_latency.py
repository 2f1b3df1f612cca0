#!/usr/bin/env python3
"""Wall time per push of the live tracker (aar_tracker_push, and aar_tracker_push_detections beside the per-frame Initializer it replaces) beside the whole-recording API used one frame at a time
(aar_problem_create of a one-frame problem + aar_track + aar_problem_destroy), on the frames of the tracking versions of configs 3 and 5.
Not part of bench.py.  Run on the MI355X:

    python scripts/live_latency.py > profiles/live_latency.txt
    rocprofv3 --kernel-trace --stats -d <dir> -- python scripts/live_latency.py --configs 3     # kernel time and call count of k_live_push

Every push is ONE launch of k_live_push (aar_tracker_push issues nothing else); the script prints the number of pushes it made, the kernel
trace's call count of k_live_push must equal it.

    python scripts/live_latency.py --gate       # every tracker a second time with the gate on, push by push beside the
                                                # ungated one (same build, same frames, interleaved); prints the added time per push
    python scripts/live_latency.py --motion     # every smoothed tracker a second time with the constant-velocity model,
                                                # interleaved in the same way (k_live_push_cv in place of k_live_push)
"""
import argparse
import contextlib
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "automatic-ar_amd"))
import aar  # noqa: E402


def ns(ds):
    return 6 * (ds.num_cams - 1) + 6 * (ds.num_markers - 1)


def one_frame(ds, f, x0):
    out = aar.Dataset.__new__(aar.Dataset)
    out.__dict__.update(ds.__dict__)
    sel = np.asarray(ds.obs_frame) == f
    out.num_frames, out.frame_ids = 1, ds.frame_ids[f:f + 1]
    out.obs_frame, out.obs_cam, out.obs_marker, out.obs_uv = np.zeros(int(sel.sum()), np.int32), ds.obs_cam[sel], ds.obs_marker[sel], ds.obs_uv[sel]
    out.num_obs = int(sel.sum())
    out.x_full = np.r_[x0[:ns(ds)], x0[ns(ds) + 6 * f: ns(ds) + 6 * f + 6]]
    return out


def stats(t):
    t = 1e6 * np.asarray(t)
    return "%8.1f us  (%.1f ... %.1f)" % (np.median(t), t.min(), t.max())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", type=int, nargs="+", default=[3, 5])
    ap.add_argument("--pushes", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--gate", action="store_true", help="also run every tracker gated (k_median 6, min_px 3), interleaved with the ungated one")
    ap.add_argument("--motion", action="store_true", help="also run every smoothed tracker with the constant-velocity motion model, interleaved")
    a = ap.parse_args()
    n = a.pushes + a.warmup
    total = total_det = 0
    for cfg in a.configs:
        ds = aar.synth(cfg, num_frames=n)
        x0 = np.array(ds.x_full)
        x0[:ns(ds)] = ds.x_truth[:ns(ds)]            # tracking: cameras and markers known, the frames at their perturbed starts
        sol = aar.Dataset.__new__(aar.Dataset)
        sol.__dict__.update(ds.__dict__)
        sol.x_full = x0
        z0 = x0[ns(ds):].reshape(-1, 6)
        obs = []
        for f in range(n):
            sel = np.asarray(ds.obs_frame) == f
            obs.append((ds.obs_cam[sel], ds.obs_marker[sel], ds.obs_uv[sel]))
        most = max(len(o[0]) for o in obs)
        print("config %d: %d cameras, %d markers, %.1f detections per frame (at most %d), %d pushes after %d warm-up" % (
            cfg, ds.num_cams, ds.num_markers, ds.num_obs / n, most, a.pushes, a.warmup))
        for label, kw in (("smooth 0", dict(lag=0, smooth=False)), ("smooth 1 lag 0", dict(lag=0, smooth=True)),
                          ("smooth 1 lag 4", dict(lag=4, smooth=True)), ("smooth 1 lag 15", dict(lag=15, smooth=True)),
                          # the tail instance of k_live_push (still one launch per push)
                          ("lag 4 marginal", dict(lag=4, smooth=True, anchor="marginal")),
                          ("lag 4 covariance", dict(lag=4, smooth=True, covariance=True)),
                          ("lag 4 both", dict(lag=4, smooth=True, anchor="marginal", covariance=True)),
                          ("lag 15 marginal", dict(lag=15, smooth=True, anchor="marginal")),
                          ("lag 15 covariance", dict(lag=15, smooth=True, covariance=True)),
                          ("lag 15 both", dict(lag=15, smooth=True, anchor="marginal", covariance=True)),
                          ("smooth 0 covar.", dict(lag=0, smooth=False, covariance=True))):
            if kw["smooth"]:
                kw.update(sigma_rot=0.05, sigma_trans=0.02)
            wall, lib, its = [], [], []
            gwall, kept, mwall, mits = [], [], [], []
            with contextlib.ExitStack() as stack:
                t = stack.enter_context(aar.Tracker(sol, max_obs_per_frame=most, **kw))
                tg = stack.enter_context(aar.Tracker(sol, max_obs_per_frame=most, gate={} if a.gate else None, **kw))
                tm = stack.enter_context(aar.Tracker(sol, max_obs_per_frame=most, motion="cv", **kw)) if a.motion and kw["smooth"] else None
                for f in range(n):
                    t0 = time.perf_counter()
                    g = t.push(float(f), *obs[f], pose_init=z0[f])
                    wall.append(time.perf_counter() - t0)
                    lib.append(g["seconds"])
                    its.append(g["iterations"])
                    total += 1
                    if a.gate:
                        t0 = time.perf_counter()
                        tg.push(float(f), *obs[f], pose_init=z0[f])
                        gwall.append(time.perf_counter() - t0)
                        kept.append(tg.last_gate()["n_kept"] / max(len(obs[f][0]), 1))
                    if a.motion and kw["smooth"]:
                        t0 = time.perf_counter()
                        g = tm.push(float(f), *obs[f], pose_init=z0[f])
                        mwall.append(time.perf_counter() - t0)
                        mits.append(g["iterations"])
            w = a.warmup
            print("  %-16s push %s   inside the library %s   %.1f LM iterations per push" % (label, stats(wall[w:]), stats(lib[w:]), np.mean(its[w:])))
            if a.gate:
                print("  %-16s push %s   gate adds %.1f us per push (difference of the medians), %.1f%% of the detections kept" % (
                    "  + gate", stats(gwall[w:]), 1e6 * (np.median(gwall[w:]) - np.median(wall[w:])), 100 * np.mean(kept[w:])))
            if a.motion and kw["smooth"]:
                print("  %-16s push %s   motion model adds %.1f us per push (difference of the medians), %.1f LM iterations per push" % (
                    "  + motion cv", stats(mwall[w:]), 1e6 * (np.median(mwall[w:]) - np.median(wall[w:])), np.mean(mits[w:])))
        frames = [one_frame(ds, f, x0) for f in range(n)]
        wall, its = [], []
        prm = aar.lm_default_params()
        for f in range(n):
            t0 = time.perf_counter()
            with aar.Problem(frames[f]) as p:
                _, it, _ = p.track(frames[f].x_full, prm)
            wall.append(time.perf_counter() - t0)
            its.append(int(it[0]))
        print("  %-16s      %s   (aar_problem_create + aar_track + aar_problem_destroy per frame)   %.1f LM iterations per frame" % (
            "create+track", stats(wall[a.warmup:]), np.mean(its[a.warmup:])))
        # raw detections: aar_tracker_push_detections under policy VOTE beside what it replaces, the Initializer on a
        # one-frame detection set with the map fixed (aar_initializer_object_poses) followed by aar_tracker_push from its pose
        K = ds.cam_mats.reshape(-1, 3, 3)
        dists = [np.zeros(5)] * ds.num_cams
        wall, its, cands, gwall = [], [], [], []
        with aar.Tracker(sol, max_obs_per_frame=most) as t, aar.Tracker(sol, max_obs_per_frame=most, gate={} if a.gate else None) as tg:
            t.enable_detections(Ks=K, dists=dists, start_policy="vote")
            tg.enable_detections(Ks=K, dists=dists, start_policy="vote")
            for f in range(n):
                t0 = time.perf_counter()
                g, info = t.push_detections(float(f), *obs[f])
                wall.append(time.perf_counter() - t0)
                its.append(g["iterations"])
                cands.append(info["candidates"])
                total_det += 1
                if a.gate:
                    t0 = time.perf_counter()
                    tg.push_detections(float(f), *obs[f])
                    gwall.append(time.perf_counter() - t0)
        w = a.warmup
        print("  %-16s push %s   %.1f candidates, %.1f LM iterations per push" % ("detections vote", stats(wall[w:]), np.mean(cands[w:]), np.mean(its[w:])))
        if a.gate:
            print("  %-16s push %s   gate adds %.1f us per push (difference of the medians)" % (
                "  + gate", stats(gwall[w:]), 1e6 * (np.median(gwall[w:]) - np.median(wall[w:]))))
        wall, its = [], []
        with aar.Tracker(sol, max_obs_per_frame=most) as t:
            for f in range(n):
                cam, mk, uv = obs[f]
                t0 = time.perf_counter()
                det = aar.Detections(int(ds.cam_ids.max()) + 1, 1, np.zeros(len(cam), np.int32), ds.cam_ids[cam], ds.marker_ids[mk], uv)
                one = aar.initializer_run(det, K, dists, ds.marker_size, solution=sol)
                g = t.push(float(f), one.obs_cam, one.obs_marker, one.obs_uv, pose_init=one.x_full[ns(ds):ns(ds) + 6])
                wall.append(time.perf_counter() - t0)
                its.append(g["iterations"])
        print("  %-16s      %s   (aar_initializer_object_poses on one frame + aar_tracker_push)   %.1f LM iterations per push" % (
            "init+push", stats(wall[w:]), np.mean(its[w:])))
    print("detection pushes made: %d; launches per detection push: 2 (k_live_init, k_live_push)" % total_det)
    print("pushes made: %d; launches per push: 1 (k_live_push; its call count in a kernel trace of this script equals the pushes made)" % total)


if __name__ == "__main__":
    main()
