#!/usr/bin/env python3
"""Wall time of aar_track_smooth_fit2 under the constant-velocity prior beside the same EM loop composed from the public
calls -- track_smooth under the model, then track_smooth_covariance2, the terms formed in numpy from the blocks it returns, the M-step on the
host -- on the same inputs: the tracking versions of configs 3, 4 and 5 (500 / 2000 / 5000 frames), started from aar_track's result.  Both
loops run a fixed number of EM iterations (rel_tol = 0) and end with one smoothing at the fitted values.  DESIGN.md section 16's method: 7
repeats after 2 warm-up calls, median (min ... max).  Not part of bench.py.  Run on the MI355X:

    python scripts/smooth_cv_fit_latency.py > profiles/smooth_cv_fit.txt
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "automatic-ar_amd"))
import aar  # noqa: E402
from smooth_fit_latency import FRAMES, left_jacobian, right_jacobian_inverse, so3_exp, so3_log, stats, timed  # noqa: E402

SROT, STRANS, SROT0, STRANS0 = 0.05, 0.02, 1.0, 1.0


def T(M):
    return np.swapaxes(M, 1, 2)


def tr_ww(X, S, Y):
    return np.einsum("nii->n", X @ S[:, :3, :3] @ T(Y))


def tr_tt(S):
    return np.einsum("nii->n", S[:, 3:, 3:])


def numpy_terms(z, fc, lc, l2, er0, et0):
    """A_r, U_r, A_t, U_t over the terms 1 .. F-2 and u_0 of a track on unit frame times (r_f = 1), vectorised (DESIGN.md sections 31, 33)"""
    wp, wc, wn = z[:-2, :3], z[1:-1, :3], z[2:, :3]
    Rp, Rc, Rn = so3_exp(wp), so3_exp(wc), so3_exp(wn)
    psi = so3_log(T(Rp) @ Rc)
    Q = T(so3_exp(psi)) @ T(Rc) @ Rn
    phi = so3_log(Q)
    Ji = right_jacobian_inverse(phi)
    B = Ji @ T(Q) @ T(left_jacobian(psi)) @ right_jacobian_inverse(psi)     # J_r(x) = J_l(x)^T
    Mn = Ji @ T(left_jacobian(wn))
    Mc = -Ji @ T(Rn) @ left_jacobian(wc) - B @ T(left_jacobian(wc))
    Mp = B @ T(Rc) @ left_jacobian(wp)
    Spp, Scc, Snn, Spc, Scn, Spn = fc[:-2], fc[1:-1], fc[2:], lc[:-1], lc[1:], l2
    ur = (tr_ww(Mp, Spp, Mp) + tr_ww(Mc, Scc, Mc) + tr_ww(Mn, Snn, Mn) + 2 * tr_ww(Mp, Spc, Mc) + 2 * tr_ww(Mc, Scn, Mn) + 2 * tr_ww(Mp, Spn, Mn))
    ut = tr_tt(Spp) + 4 * tr_tt(Scc) + tr_tt(Snn) - 4 * tr_tt(Spc) - 4 * tr_tt(Scn) + 2 * tr_tt(Spn)
    et = z[2:, 3:] - 2 * z[1:-1, 3:] + z[:-2, 3:]
    # pair 0 in the random walk's form
    R0, R1 = so3_exp(z[:1, :3]), so3_exp(z[1:2, :3])
    J0 = right_jacobian_inverse(so3_log(T(R0) @ R1))
    Mb = J0 @ T(left_jacobian(z[1:2, :3]))
    Ma = -J0 @ T(R1) @ left_jacobian(z[:1, :3])
    u0r = tr_ww(Ma, fc[:1], Ma) + tr_ww(Mb, fc[1:2], Mb) + 2 * tr_ww(Ma, lc[:1], Mb)
    u0t = tr_tt(fc[:1]) + tr_tt(fc[1:2]) - 2 * tr_tt(lc[:1])
    return np.array([np.sum(phi * phi), np.sum(ur), np.sum(et * et), np.sum(ut)]), float(u0r[0] / er0 ** 2 + u0t[0] / et0 ** 2)


def composed_fit(p, x0, n0, F, N, iters):
    """the loop of aar_track_smooth_fit2 from the public calls: every iteration uploads the track, allocates its workspaces and brings the blocks
    back to the host"""
    q, s_r, s_t = 1.0, SROT ** 2, STRANS ** 2
    er, et, er0, et0 = SROT, STRANS, SROT0, STRANS0
    x = x0
    for _ in range(iters):
        cv = dict(model=1, sigma_rot0=er0, sigma_trans0=et0)
        x, _, _, _ = p.track_smooth(x, er, et, **cv)
        fc, lc, l2, rep = p.track_smooth_covariance2(x, er, et, **cv)
        (A_r, U_r, A_t, U_t), u_0 = numpy_terms(x[n0:n0 + 6 * F].reshape(F, 6), fc, lc, l2, er0, et0)
        U_d = 6.0 * F - U_r / (er * er) - U_t / (et * et) - u_0
        s_r, s_t, q = (A_r + q * U_r) / (3.0 * (F - 2)), (A_t + q * U_t) / (3.0 * (F - 2)), (rep["data_cost"] + q * U_d) / (8.0 * N)
        er, et, er0, et0 = np.sqrt(s_r / q), np.sqrt(s_t / q), SROT0 / np.sqrt(q), STRANS0 / np.sqrt(q)
    x, _, _, _ = p.track_smooth(x, er, et, model=1, sigma_rot0=er0, sigma_trans0=et0)
    return x, np.sqrt([q, s_r, s_t])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", type=int, nargs="+", default=[3, 4, 5])
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--iters", type=int, default=10, help="EM iterations of both loops")
    a = ap.parse_args()
    cv = dict(model=1, sigma_rot0=SROT0, sigma_trans0=STRANS0)
    for cfg in a.configs:
        F = FRAMES[cfg]
        ds = aar.synth(cfg, num_frames=F)
        n0 = 6 * (ds.num_cams - 1) + 6 * (ds.num_markers - 1)
        x0 = np.array(ds.x_full)
        x0[:n0] = ds.x_truth[:n0]
        fit = dict(max_iters=a.iters, rel_tol=0.0)
        with aar.Problem(ds) as p:
            xt, _, _ = p.track(x0, aar.lm_default_params())
            _, rep, path = p.track_smooth_fit2(xt, SROT, STRANS, fit=fit, **cv)
            _, sig = composed_fit(p, xt, n0, F, ds.num_obs, a.iters)
            t_fit = timed(lambda: p.track_smooth_fit2(xt, SROT, STRANS, fit=fit, **cv), a.warmup, a.repeats)
            t_cmp = timed(lambda: composed_fit(p, xt, n0, F, ds.num_obs, a.iters), a.warmup, a.repeats)
            _, conv, _ = p.track_smooth_fit2(xt, SROT, STRANS, **cv)
        agree = float(np.max(np.abs(sig / path[-1] - 1.0)))
        print("config %d, F = %d, %d detections, %d EM iterations, constant velocity: aar_track_smooth_fit2 %s = %.3f ms per iteration, %d LM steps, "
              "%d launches; composed from the public calls %s = %.3f ms per iteration; sigmas (px, rot, trans) %s, the composed loop's differ by "
              "%.1e; default fit: %d iterations (exit %d), sigma_px %.4f sigma_rot %.5f sigma_trans %.5f"
              % (cfg, F, ds.num_obs, a.iters, stats(t_fit), 1e3 * np.median(t_fit) / a.iters, rep["lm_steps"], rep["launches"], stats(t_cmp),
                 1e3 * np.median(t_cmp) / a.iters, np.array2string(path[-1], precision=5), agree, conv["iterations"], conv["stop_code"],
                 conv["sigma_px"], conv["sigma_rot"], conv["sigma_trans"]), flush=True)


if __name__ == "__main__":
    main()
