#!/usr/bin/env python3
"""Wall time of the per-detection layer of a smoothed track on the tracking versions of configs 3, 4 and 5 (500 / 2000 /
5000 frames, the configs' own detections per frame), under both motion models, at aar_track_smooth's result started from aar_track's:
  - aar_track_smooth_detection_leverage and aar_track_smooth_detection_loo over the problem's detections;
  - aar_track_smooth_predict_corners (with cov) and aar_track_smooth_gate_detections at the detections' own (camera, marker, frame time);
  - aar_track_smooth_covariance2 alone on the same input: the chain every entry pays;
  - k_smooth_corners' own time between two HIP events (the reports' kernel_seconds, aar_set_kernel_profiling on, a run of its own), per
    launch and per detection.
As context, not as a bar: the bundle's k_predict_corners spends (detection_leverage - aar_problem_covariance alone) / detections =
(110.774 - 8.185) ms / 1258587 = 81.5 ns per detection at config 5 (profiles/predict_latency.txt; gains launch and copies included).
DESIGN.md section 16's method: 7 repeats after 2 warm-up calls, median (min ... max), host copies of the outputs included.  Not part of
bench.py.  Run on the MI355X:

    python scripts/smooth_loo_latency.py > profiles/smooth_loo_latency.txt
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
MODELS = {"rw": dict(model="rw"), "cv": dict(model="cv", sigma_rot0=1.0, sigma_trans0=1.0)}
FRAMES = {3: 500, 4: 2000, 5: 5000}
PREDICT_NS = (110.774 - 8.185) * 1e6 / 1258587          # profiles/predict_latency.txt, config 5


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
        N = ds.num_obs
        n0 = 6 * (ds.num_cams - 1) + 6 * (ds.num_markers - 1)
        x0 = np.array(ds.x_full)
        x0[:n0] = ds.x_truth[:n0]
        qc, qm, qt = np.asarray(ds.obs_cam), np.asarray(ds.obs_marker), np.asarray(ds.obs_frame, dtype=np.float64)
        obs = np.asarray(ds.obs_uv, dtype=np.float32).reshape(-1, 8)
        for name, kw in MODELS.items():
            with aar.Problem(ds) as p:
                xt, _, _ = p.track(x0, aar.lm_default_params())
                xs = p.track_smooth(xt, SROT, STRANS, **kw)[0]
                calls = {
                    "detection_leverage": lambda: p.track_smooth_detection_leverage(xs, SROT, STRANS, rows=True, **kw)[2],
                    "detection_loo": lambda: p.track_smooth_detection_loo(xs, SROT, STRANS, f_max=3.27, **kw).report,
                    "predict_corners": lambda: p.track_smooth_predict_corners(xs, SROT, STRANS, qc, qm, qt, **kw)[4],
                    "gate_detections": lambda: p.track_smooth_gate_detections(xs, SROT, STRANS, qc, qm, qt, obs, **kw)[4],
                }
                wall = {k: timed(fn, a.warmup, a.repeats) for k, fn in calls.items()}
                t_c = timed(lambda: p.track_smooth_covariance2(xs, SROT, STRANS, lag2=name == "cv", **kw), a.warmup, a.repeats)
                rep = calls["detection_loo"]()
                launches = {k: fn()["launches"] for k, fn in calls.items()}
                # the kernel's own time: a run of its own with the events on
                p.set_kernel_profiling(True)
                kern = {}
                for k, fn in calls.items():
                    for _ in range(a.warmup):
                        fn()
                    kern[k] = [fn()["kernel_seconds"] for _ in range(a.repeats)]
                p.set_kernel_profiling(False)
            print("config %d, F = %d, %d detections (%.1f per frame), %s: aar_track_smooth_covariance2 alone %s; largest F %.3f, %d above 3.27, %d undetermined"
                  % (cfg, F, N, N / F, name, stats(t_c), rep["max_f"], rep["rejected"], rep["undetermined"]), flush=True)
            for k in calls:
                ks = np.median(kern[k])
                print("config %d, %s, %s: %s, %d launches; k_smooth_corners %s = %.2f ns per detection (k_predict_corners, the bundle, config 5: %.1f ns)"
                      % (cfg, name, k, stats(wall[k]), launches[k], stats(kern[k]), 1e9 * ks / N, PREDICT_NS), flush=True)


if __name__ == "__main__":
    main()
