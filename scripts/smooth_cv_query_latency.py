#!/usr/bin/env python3
"""Wall time of aar_track_smooth_query2 under the constant-velocity prior on the tracking versions of configs 3, 4 and
5 (500 / 2000 / 5000 frames), at aar_track_smooth's result started from aar_track's, with Q = 10 (F - 1) + 1 evenly spaced query times
(every gap cut in ten, the frames included).  Beside it, on the same inputs:
  - the same call without the copy of the blocks (cov = NULL: the same chain);
  - aar_track_smooth_covariance2 alone, whose chain the query contains;
  - the composition from public calls: one aar_track_smooth_covariance2 per query on a data set with a frame without detections inserted at
    the query's time and start pose, timed for 16 queries spread over the sequence (the problem of each built outside the timed region)
    and extrapolated to Q.  (That yields the block alone; the pose would take a solve on top.)
DESIGN.md section 16's method: 7 repeats after 2 warm-up calls, median (min ... max).  Not part of bench.py.  Run on the MI355X:

    python scripts/smooth_cv_query_latency.py > profiles/smooth_cv_query.txt
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "automatic-ar_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import aar  # noqa: E402
import smooth_cv_query_cases as cqc  # noqa: E402

SROT, STRANS = 0.05, 0.02
CV = dict(model="cv", sigma_rot0=1.0, sigma_trans0=1.0)
FRAMES = {3: 500, 4: 2000, 5: 5000}


def stats(t):
    t = 1e3 * np.asarray(t)
    return "%.3f ms (%.3f ... %.3f)" % (np.median(t), t.min(), t.max())


def timed(fn, warmup, repeats):
    for _ in range(warmup):
        fn()
    out = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        fn()
        out.append(time.perf_counter() - t0)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", type=int, nargs="+", default=[3, 4, 5])
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--composed", type=int, default=16, help="queries timed through the composition (0: skip it)")
    a = ap.parse_args()
    for cfg in a.configs:
        F = FRAMES[cfg]
        ds = aar.synth(cfg, num_frames=F)
        n0 = 6 * (ds.num_cams - 1) + 6 * (ds.num_markers - 1)
        x0 = np.array(ds.x_full)
        x0[:n0] = ds.x_truth[:n0]
        qt = np.arange(10 * (F - 1) + 1) / 10.0           # (entry 10 f is frame f's time exactly)
        with aar.Problem(ds) as p:
            xt, _, _ = p.track(x0, aar.lm_default_params())
            xs, _, _, _ = p.track_smooth(xt, SROT, STRANS, **CV)
            pose, cov, seg, rep = p.track_smooth_query2(xs, SROT, STRANS, qt, **CV)
            start, _ = p.track_smooth_query2_step(xs, SROT, STRANS, qt, **CV)
            t_q = timed(lambda: p.track_smooth_query2(xs, SROT, STRANS, qt, **CV), a.warmup, a.repeats)
            t_p = timed(lambda: p.track_smooth_query2(xs, SROT, STRANS, qt, covariance=False, **CV), a.warmup, a.repeats)
            t_c = timed(lambda: p.track_smooth_covariance2(xs, SROT, STRANS, **CV), a.warmup, a.repeats)
        line = ("config %d, F = %d, %d detections, Q = %d (%d inside, %d on frames): aar_track_smooth_query2 %s, %d launches; without the copy "
                "of the blocks %s; aar_track_smooth_covariance2 alone %s" % (cfg, F, ds.num_obs, len(qt), rep["num_inside"], rep["num_on_frame"],
                                                                            stats(t_q), rep["launches"], stats(t_p), stats(t_c)))
        if a.composed:
            idx = np.nonzero(seg * 1.0 != qt)[0]              # not on a frame time
            pick = idx[np.linspace(0, len(idx) - 1, a.composed).astype(int)]
            each, worst = [], 0.0
            for k in pick:
                ds2, x2, ft2, pos = cqc.inserted(ds, xs, None, float(qt[k]), zm=start[k])
                with aar.Problem(ds2) as p2:
                    S2 = p2.track_smooth_covariance2(x2, SROT, STRANS, frame_time=ft2, **CV)[0]
                    each.append(np.median(timed(lambda: p2.track_smooth_covariance2(x2, SROT, STRANS, frame_time=ft2, **CV), 1, 3)))
                worst = max(worst, float(np.linalg.norm(cov[k] - S2[pos]) / np.linalg.norm(S2[pos])))
            per = float(np.median(each))
            line += ("; composed from aar_track_smooth_covariance2 on an augmented data set: %.3f ms per query over %d queries = %.1f s for Q "
                     "(%.0f x the call), largest difference of a block %.1e" % (1e3 * per, len(pick), per * len(qt), per * len(qt) / np.median(t_q), worst))
        print(line, flush=True)


if __name__ == "__main__":
    main()
