// The live tracker's constant-velocity motion model on the host: the expected motion of a new pair from the two newest
// estimates, the prediction the new frame starts from, the velocity aar_tracker_predict extrapolates with.  fp64, no device code: the kernels
// only receive the results (csrc/kernels.h, LiveMotionArgs).
#pragma once
#include <cmath>

#include "se3.h"

namespace aar {

// log(Q)^v of a rotation matrix, as csrc/so3.hpp in all three branches: theta from atan2 (exact at small angles, where cv::Rodrigues' matrix ->
// vector gives 0); near pi the axis from the symmetric part (Q + Q^T) / 2 - cos(theta) I = (1 - cos(theta)) n n^T, its sign from v.
// (rodrigues_mat2vec is the reference's cv::Rodrigues, not this: its theta comes from acos, and below sin(theta) = 1e-5 it takes the axis from
// the diagonal alone with OpenCV's sign rule -- off by up to twice the distance to pi for a board that faces the root camera.)
inline void motion_so3_log(const double Q[9], double phi[3]) {
    const double v0 = Q[7] - Q[5], v1 = Q[2] - Q[6], v2 = Q[3] - Q[1];
    const double s2 = std::sqrt(v0 * v0 + v1 * v1 + v2 * v2);   // 2 sin(theta)
    const double c = 0.5 * (Q[0] + Q[4] + Q[8] - 1.0);
    const double theta = std::atan2(0.5 * s2, c);
    if (c > -0.99) {
        const double k = theta < 1e-4 ? 0.5 + theta * theta * (1.0 / 12.0) : theta / s2;
        phi[0] = k * v0; phi[1] = k * v1; phi[2] = k * v2;
        return;
    }
    const double oc = 1.0 - c;
    const double d0 = (Q[0] - c) / oc, d1 = (Q[4] - c) / oc, d2 = (Q[8] - c) / oc;   // n_i^2
    double n0, n1, n2;
    if (d0 >= d1 && d0 >= d2) {
        n0 = std::sqrt(std::fmax(d0, 0.0));
        n1 = 0.5 * (Q[1] + Q[3]) / (oc * n0); n2 = 0.5 * (Q[2] + Q[6]) / (oc * n0);
    } else if (d1 >= d2) {
        n1 = std::sqrt(std::fmax(d1, 0.0));
        n0 = 0.5 * (Q[1] + Q[3]) / (oc * n1); n2 = 0.5 * (Q[5] + Q[7]) / (oc * n1);
    } else {
        n2 = std::sqrt(std::fmax(d2, 0.0));
        n0 = 0.5 * (Q[2] + Q[6]) / (oc * n2); n1 = 0.5 * (Q[5] + Q[7]) / (oc * n2);
    }
    const double in = 1.0 / std::sqrt(n0 * n0 + n1 * n1 + n2 * n2);
    const double sg = (n0 * v0 + n1 * v1 + n2 * v2) < 0.0 ? -1.0 : 1.0;
    phi[0] = sg * theta * n0 * in; phi[1] = sg * theta * n1 * in; phi[2] = sg * theta * n2 * in;
}

// (omega, v) of the pair (a, b): omega = log(R_a^T R_b) in the body frame of a, v = t_b - t_a in the root camera's frame
inline void motion_between(const double za[6], const double zb[6], double wv[6]) {
    double Ra[9], Rb[9], Rat[9], Q[9];
    rodrigues_vec2mat(za, Ra);
    rodrigues_vec2mat(zb, Rb);
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) Rat[3 * i + j] = Ra[3 * j + i];
    mat3_mul(Rat, Rb, Q);
    motion_so3_log(Q, wv);
    for (int k = 0; k < 3; k++) wv[3 + k] = zb[3 + k] - za[3 + k];
}

// the pose z moved by (omega, v): (R exp(omega), t + v) as (rvec, t)
inline void motion_apply(const double z[6], const double wv[6], double out[6]) {
    double R[9], E[9], Q[9];
    rodrigues_vec2mat(z, R);
    rodrigues_vec2mat(wv, E);
    mat3_mul(R, E, Q);
    motion_so3_log(Q, out);
    for (int k = 0; k < 3; k++) out[3 + k] = z[3 + k] + wv[3 + k];
}

// The state a tracker with the model carries from push to push: the two newest estimates as the last accepted push left them and their times.
struct MotionState {
    int frames = 0;            // estimates held: 0, 1 or 2
    double za[6], zb[6];       // frame n - 2 (frames == 2), frame n - 1 (frames >= 1)
    double ta = 0, tb = 0;
};

// The rule of push n at frame_time: rel_n = s (omega, v) of the pair (a, b), s = (time - tb) / (tb - ta); zero before two frames and, with
// max_dt > 0, when either gap exceeds it.  pred: zb moved by rel (zb itself, bit for bit, where rel is zero).  Returns whether rel was measured.
inline bool motion_measure(const MotionState &m, double frame_time, double max_dt, double rel[6], double pred[6]) {
    for (int k = 0; k < 6; k++) { rel[k] = 0.0; pred[k] = m.frames >= 1 ? m.zb[k] : 0.0; }
    if (m.frames < 2) return false;
    const double g0 = m.tb - m.ta, g1 = frame_time - m.tb;
    if (max_dt > 0.0 && (g0 > max_dt || g1 > max_dt)) return false;
    double wv[6];
    motion_between(m.za, m.zb, wv);
    const double s = g1 / g0;
    for (int k = 0; k < 6; k++) rel[k] = s * wv[k];
    motion_apply(m.zb, rel, pred);
    return true;
}

// (omega, v) per unit of time of the newest pair; zeros before two frames
inline void motion_velocity(const MotionState &m, double vel[6]) {
    for (int k = 0; k < 6; k++) vel[k] = 0.0;
    if (m.frames < 2) return;
    double wv[6];
    motion_between(m.za, m.zb, wv);
    for (int k = 0; k < 6; k++) vel[k] = wv[k] / (m.tb - m.ta);
}

// the newest pose extrapolated to time >= tb; the newest pose itself past max_dt (> 0) or before two frames
inline void motion_predict(const MotionState &m, double time, double max_dt, double pose[6]) {
    for (int k = 0; k < 6; k++) pose[k] = m.zb[k];
    const double d = time - m.tb;
    if (m.frames < 2 || !(d > 0.0) || (max_dt > 0.0 && d > max_dt)) return;
    double vel[6], wv[6];
    motion_velocity(m, vel);
    for (int k = 0; k < 6; k++) wv[k] = d * vel[k];
    motion_apply(m.zb, wv, pose);
}

}  // namespace aar
