#!/usr/bin/env python3
"""Wall time of aar_track_smooth_covariance2 under the constant-velocity prior beside aar_track_smooth_system2 with its
solve at mu = 0 on the same inputs in the same process (what the downward pass adds), and beside the random walk's aar_track_smooth_covariance:
the tracking versions of configs 3, 4 and 5 (500 / 2000 / 5000 frames), at aar_track_smooth's constant-velocity result started from aar_track's.
DESIGN.md section 16's method: 7 repeats after 2 warm-up calls, median (min ... max).  Not part of bench.py.  Run on the MI355X:

    python scripts/smooth_cv_covariance_latency.py > profiles/smooth_cv_covariance.txt
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "automatic-ar_amd"))
import aar  # noqa: E402

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
    a = ap.parse_args()
    for cfg in a.configs:
        F = FRAMES[cfg]
        ds = aar.synth(cfg, num_frames=F)
        n0 = 6 * (ds.num_cams - 1) + 6 * (ds.num_markers - 1)
        x0 = np.array(ds.x_full)
        x0[:n0] = ds.x_truth[:n0]
        with aar.Problem(ds) as p:
            xt, _, _ = p.track(x0, aar.lm_default_params())
            xs, _, _, _ = p.track_smooth(xt, SROT, STRANS, **CV)
            S, R, R2, rep = p.track_smooth_covariance2(xs, SROT, STRANS, **CV)
            t_cov = timed(lambda: p.track_smooth_covariance2(xs, SROT, STRANS, **CV), a.warmup, a.repeats)
            t_sys = timed(lambda: p.track_smooth_system2(xs, SROT, STRANS, 0.0, **CV), a.warmup, a.repeats)
            _, _, rw = p.track_smooth_covariance(xs, SROT, STRANS)
            t_rw = timed(lambda: p.track_smooth_covariance(xs, SROT, STRANS), a.warmup, a.repeats)
        s1 = np.sqrt(rep["sigma2"] * np.einsum("fii->f", S[:, 3:, 3:]))
        print("config %d, F = %d, %d detections: aar_track_smooth_covariance2 (constant velocity) %s, %d launches; aar_track_smooth_system2 with its "
              "solve at mu = 0 %s; aar_track_smooth_covariance (random walk) %s, %d launches; sigma2 %.4f, 1-sigma translation %.3e ... %.3e m" %
              (cfg, F, ds.num_obs, stats(t_cov), rep["launches"], stats(t_sys), stats(t_rw), rw["launches"], rep["sigma2"], s1.min(), s1.max()),
              flush=True)


if __name__ == "__main__":
    main()
