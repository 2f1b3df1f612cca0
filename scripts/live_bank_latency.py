#!/usr/bin/env python3
"""Wall time per push of the tracker bank (aar_tracker_bank_push: one copy in, one launch of B workgroups, one copy out) beside B sequential
aar_tracker_push calls on the same frames, at B = 1, 8, 64, 256, with the bytes copied per push (aar_tracker_bank_get_stats).
Not part of bench.py.  Run on the MI355X:

    python scripts/live_bank_latency.py > profiles/live_bank_latency.txt

Every member tracks the object of config 3's tracking version; member b is fed the recording shifted by 7 b frames, so that the members' inputs
differ.  Times are taken around the library calls alone (the arrays are laid out beforehand).  The script's one condition, checked at the end:
at B = 8 the median bank push lies below the median of the eight sequential pushes together.

    python scripts/live_bank_latency.py --gate      # a second, gated bank pushed beside the ungated one, push by push
                                                    # (same build, same frames, interleaved); prints the added time per push
"""
import argparse
import ctypes as C
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "automatic-ar_amd"))
import aar  # noqa: E402


def ns(ds):
    return 6 * (ds.num_cams - 1) + 6 * (ds.num_markers - 1)


def stats(t):
    t = 1e6 * np.asarray(t)
    return "%9.1f us  (%.1f ... %.1f)" % (np.median(t), t.min(), t.max())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--members", type=int, nargs="+", default=[1, 8, 64, 256])
    ap.add_argument("--pushes", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--gate", action="store_true", help="also push a gated bank (k_median 6, min_px 3), interleaved with the ungated one")
    ap.add_argument("--motion", action="store_true", help="also push every smoothed bank with the constant-velocity motion model (DESIGN.md section 25), interleaved")
    ap.add_argument("--lags", type=int, nargs="+", default=[4], help="lags of the smoothed banks")
    a = ap.parse_args()
    n, w = a.pushes + a.warmup, a.warmup
    ds = aar.synth(3, num_frames=n)
    x0 = np.array(ds.x_full)
    x0[:ns(ds)] = ds.x_truth[:ns(ds)]                # tracking: cameras and markers known, the frames at their perturbed starts
    sol = aar.Dataset.__new__(aar.Dataset)
    sol.__dict__.update(ds.__dict__)
    sol.x_full = x0
    z0 = x0[ns(ds):].reshape(-1, 6)
    obs = []
    for f in range(n):
        sel = np.asarray(ds.obs_frame) == f
        obs.append((ds.obs_cam[sel], ds.obs_marker[sel], ds.obs_uv[sel]))
    most = max(len(o[0]) for o in obs)
    print("config 3: %d cameras, %d markers, %.1f detections per frame (at most %d), %d pushes after %d warm-up" % (
        ds.num_cams, ds.num_markers, ds.num_obs / n, most, a.pushes, w))
    L = aar.lib()
    ip, fp, dp = C.POINTER(C.c_int32), C.POINTER(C.c_float), C.POINTER(C.c_double)
    medians = {}
    modes = [("smooth 0", dict(lag=0, smooth=False))] + [("smooth 1 lag %d" % lag, dict(lag=lag, smooth=True, sigma_rot=0.05, sigma_trans=0.02)) for lag in a.lags]
    for label, kw in modes:
        print("%s" % label)
        for B in a.members:
            src = [[(f + 7 * b) % n for b in range(B)] for f in range(n)]           # the recording's frame member b is fed at push f
            # ---- the bank ----
            wall, gwall, mwall = [], [], []
            mot = a.motion and kw["smooth"]
            with aar.TrackerBank([sol] * B, max_obs_per_frame=most, **kw) as k, \
                    aar.TrackerBank([sol] * (B if a.gate else 1), max_obs_per_frame=most, gate={} if a.gate else None, **kw) as kg, \
                    aar.TrackerBank([sol] * (B if mot else 1), max_obs_per_frame=most, motion="cv" if mot else None, **kw) as km:
                res, gres, mres = k.result_array(), kg.result_array(), km.result_array()
                for f in range(n):
                    args, keep = k.pack([obs[s] for s in src[f]], [z0[s] for s in src[f]])
                    t0 = time.perf_counter()
                    rc = L.aar_tracker_bank_push(k.handle, float(f), *args, res)
                    wall.append(time.perf_counter() - t0)
                    assert rc == 0, L.aar_last_error()
                    if a.gate:
                        t0 = time.perf_counter()
                        rc = L.aar_tracker_bank_push(kg.handle, float(f), *args, gres)
                        gwall.append(time.perf_counter() - t0)
                        assert rc == 0, L.aar_last_error()
                    if mot:
                        t0 = time.perf_counter()
                        rc = L.aar_tracker_bank_push(km.handle, float(f), *args, mres)
                        mwall.append(time.perf_counter() - t0)
                        assert rc == 0, L.aar_last_error()
                st = k.stats()
                gst = kg.stats()
                mst = km.stats()
                its = np.mean([r.iterations for r in res])
            # ---- what the parent offers: B trackers pushed one after the other ----
            seq = []
            trackers = [aar.Tracker(sol, max_obs_per_frame=most, **kw) for _ in range(B)]
            try:
                r = aar.CTrackerResult()
                r.struct_size = C.sizeof(aar.CTrackerResult)
                for f in range(n):
                    calls = []
                    for b, s in enumerate(src[f]):
                        cam, mk, uv = (np.ascontiguousarray(x) for x in obs[s])
                        calls.append((trackers[b].handle, float(f), len(cam), cam.ctypes.data_as(ip), mk.ctypes.data_as(ip), uv.ctypes.data_as(fp),
                                      z0[s].ctypes.data_as(dp), C.byref(r), (cam, mk, uv)))
                    t0 = time.perf_counter()
                    for c in calls:
                        rc = L.aar_tracker_push(*c[:8])
                    seq.append(time.perf_counter() - t0)
                    assert rc == 0, L.aar_last_error()
            finally:
                for t in trackers:
                    t.close()
            mb, ms = np.median(wall[w:]), np.median(seq[w:])
            medians[(label, B)] = (mb, ms)
            print("  B %4d   bank push %s   %d sequential pushes %s   ratio %.2f   copied per push: in %d bytes, out %d bytes   "
                  "launches per push %.0f   %.1f LM iterations at the last push" % (
                      B, stats(wall[w:]), B, stats(seq[w:]), ms / mb, st["h2d_bytes"] // st["pushes"], st["d2h_bytes"] // st["pushes"],
                      st["launches"] / st["pushes"], its))
            if a.gate:
                print("  B %4d   + gate    %s   gate adds %.1f us per push (difference of the medians)   copied out %d bytes   launches per push %.0f" % (
                    B, stats(gwall[w:]), 1e6 * (np.median(gwall[w:]) - mb), gst["d2h_bytes"] // gst["pushes"], gst["launches"] / gst["pushes"]))
            if mot:
                print("  B %4d   + motion  %s   motion model adds %.1f us per push (difference of the medians)   copied per push: in %d bytes, out %d bytes   "
                      "launches per push %.0f" % (B, stats(mwall[w:]), 1e6 * (np.median(mwall[w:]) - mb), mst["h2d_bytes"] // mst["pushes"],
                                                  mst["d2h_bytes"] // mst["pushes"], mst["launches"] / mst["pushes"]))
    ok = all(medians[(label, 8)][0] < medians[(label, 8)][1] for label, B in medians if B == 8)
    print("condition (B = 8: bank push median below the eight sequential pushes together): %s" % ("met" if ok else "NOT MET"))
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
