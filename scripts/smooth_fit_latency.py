#!/usr/bin/env python3
"""Wall time of aar_track_smooth_fit beside the same EM loop composed from the public calls -- track_smooth, then
track_smooth_covariance, the pairs' terms formed in numpy from the blocks it returns, the M-step on the host -- on the same inputs: the tracking
versions of configs 3, 4 and 5 (500 / 2000 / 5000 frames), started from aar_track's result.  Both loops run a fixed number of EM iterations
(rel_tol = 0) and end with one smoothing at the fitted values.  DESIGN.md section 16's method: 7 repeats after 2 warm-up calls, median
(min ... max).  Not part of bench.py.  Run on the MI355X:

    python scripts/smooth_fit_latency.py > profiles/smooth_fit.txt
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


def hat(w):
    z = np.zeros(len(w))
    return np.stack([np.stack([z, -w[:, 2], w[:, 1]], -1), np.stack([w[:, 2], z, -w[:, 0]], -1), np.stack([-w[:, 1], w[:, 0], z], -1)], -2)


def so3_exp(w):
    th = np.linalg.norm(w, axis=1)
    K = hat(w)
    small = th < 1e-6
    t = np.where(small, 1.0, th)
    a = np.where(small, 1.0 - th * th / 6, np.sin(t) / t)
    b = np.where(small, 0.5 - th * th / 24, (1 - np.cos(t)) / (t * t))
    return np.eye(3) + a[:, None, None] * K + b[:, None, None] * (K @ K)


def so3_log(Q):
    c = np.clip(0.5 * (np.einsum("nii->n", Q) - 1.0), -1.0, 1.0)
    th = np.arccos(c)
    v = np.stack([Q[:, 2, 1] - Q[:, 1, 2], Q[:, 0, 2] - Q[:, 2, 0], Q[:, 1, 0] - Q[:, 0, 1]], -1)
    k = np.where(th < 1e-6, 0.5 + th * th / 12, th / (2 * np.sin(np.where(th < 1e-6, 1.0, th))))
    return k[:, None] * v


def left_jacobian(w):
    th = np.linalg.norm(w, axis=1)
    K = hat(w)
    small = th < 1e-6
    t = np.where(small, 1.0, th)
    a = np.where(small, 0.5 - th * th / 24, (1 - np.cos(t)) / (t * t))
    b = np.where(small, 1.0 / 6 - th * th / 120, (t - np.sin(t)) / (t ** 3))
    return np.eye(3) + a[:, None, None] * K + b[:, None, None] * (K @ K)


def right_jacobian_inverse(w):
    th = np.linalg.norm(w, axis=1)
    K = hat(w)
    small = th < 1e-3
    t = np.where(small, 1.0, th)
    c = np.where(small, 1.0 / 12 + th * th / 720, 1 / (t * t) - (1 + np.cos(t)) / (2 * t * np.sin(t)))
    return np.eye(3) + 0.5 * K + c[:, None, None] * (K @ K)


def numpy_terms(z, S, R):
    """A_r, U_r, A_t, U_t of a track without frame times or expected motions, vectorised over the pairs"""
    Ra, Rb = so3_exp(z[:-1, :3]), so3_exp(z[1:, :3])
    phi = so3_log(np.swapaxes(Ra, 1, 2) @ Rb)
    Ji = right_jacobian_inverse(phi)
    Mb = Ji @ np.swapaxes(left_jacobian(z[1:, :3]), 1, 2)
    Ma = -Ji @ np.swapaxes(Rb, 1, 2) @ left_jacobian(z[:-1, :3])
    Sf, Sg, Rf = S[:-1], S[1:], R
    C = (Ma @ Sf[:, :3, :3] @ np.swapaxes(Ma, 1, 2) + Mb @ Sg[:, :3, :3] @ np.swapaxes(Mb, 1, 2) + Ma @ Rf[:, :3, :3] @ np.swapaxes(Mb, 1, 2)
         + Mb @ np.swapaxes(Rf[:, :3, :3], 1, 2) @ np.swapaxes(Ma, 1, 2))
    et = z[1:, 3:] - z[:-1, 3:]
    T = Sf[:, 3:, 3:] + Sg[:, 3:, 3:] - Rf[:, 3:, 3:] - np.swapaxes(Rf[:, 3:, 3:], 1, 2)
    return np.array([np.sum(phi * phi), np.einsum("nii->", C), np.sum(et * et), np.einsum("nii->", T)])


def composed_fit(p, x0, n0, F, N, iters):
    """the loop of aar_track_smooth_fit from the public calls: every iteration uploads the track, allocates its workspaces and brings the blocks
    back to the host"""
    q, s_r, s_t = 1.0, SROT ** 2, STRANS ** 2
    er, et = SROT, STRANS
    x = x0
    for _ in range(iters):
        x, _, _, _ = p.track_smooth(x, er, et)
        S, R, rep = p.track_smooth_covariance(x, er, et)
        A_r, U_r, A_t, U_t = numpy_terms(x[n0:n0 + 6 * F].reshape(F, 6), S, R)
        U_d = 6.0 * F - U_r / (er * er) - U_t / (et * et)
        s_r, s_t, q = (A_r + q * U_r) / (3.0 * (F - 1)), (A_t + q * U_t) / (3.0 * (F - 1)), (rep["data_cost"] + q * U_d) / (8.0 * N)
        er, et = np.sqrt(s_r / q), np.sqrt(s_t / q)
    x, _, _, _ = p.track_smooth(x, er, et)
    return x, np.sqrt([q, s_r, s_t])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", type=int, nargs="+", default=[3, 4, 5])
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--iters", type=int, default=10, help="EM iterations of both loops")
    a = ap.parse_args()
    for cfg in a.configs:
        F = FRAMES[cfg]
        ds = aar.synth(cfg, num_frames=F)
        n0 = 6 * (ds.num_cams - 1) + 6 * (ds.num_markers - 1)
        x0 = np.array(ds.x_full)
        x0[:n0] = ds.x_truth[:n0]
        fit = dict(max_iters=a.iters, rel_tol=0.0)
        with aar.Problem(ds) as p:
            xt, _, _ = p.track(x0, aar.lm_default_params())
            _, rep, path = p.track_smooth_fit(xt, SROT, STRANS, fit=fit)
            _, sig = composed_fit(p, xt, n0, F, ds.num_obs, a.iters)
            t_fit = timed(lambda: p.track_smooth_fit(xt, SROT, STRANS, fit=fit), a.warmup, a.repeats)
            t_cmp = timed(lambda: composed_fit(p, xt, n0, F, ds.num_obs, a.iters), a.warmup, a.repeats)
            _, conv, _ = p.track_smooth_fit(xt, SROT, STRANS)
        agree = float(np.max(np.abs(sig / path[-1] - 1.0)))
        print("config %d, F = %d, %d detections, %d EM iterations: aar_track_smooth_fit %s = %.3f ms per iteration, %d LM steps, %d launches; "
              "composed from the public calls %s = %.3f ms per iteration; sigmas (px, rot, trans) %s, the composed loop's differ by %.1e; "
              "default fit: %d iterations (exit %d), sigma_px %.4f sigma_rot %.5f sigma_trans %.5f"
              % (cfg, F, ds.num_obs, a.iters, stats(t_fit), 1e3 * np.median(t_fit) / a.iters, rep["lm_steps"], rep["launches"], stats(t_cmp),
                 1e3 * np.median(t_cmp) / a.iters, np.array2string(path[-1], precision=5), agree, conv["iterations"], conv["stop_code"],
                 conv["sigma_px"], conv["sigma_rot"], conv["sigma_trans"]), flush=True)


if __name__ == "__main__":
    main()
