// Device functions of the Initializer's arithmetic, shared by its own kernels (init_kernels.hip: k_ippe, k_pair_cands, k_object_cands,
// k_vote) and by the live tracker's per-frame start (live_init_kernels.hip: k_live_init):
//   undistortion + square-marker IPPE of one detection (aruco::solvePnP_, 3rdparty/aruco/aruco/ippe.cpp:118-223),
//   the 3x4 affine helpers and the candidate of fill_transformation_set (libs/initializer.cpp:73-93),
//   one (i, j) term of find_best_transformation (:151-193),
//   a 3x4 -> (rvec, t) with host/se3.h's own matrix -> vector code.
// All matrices are the 3x4 top of the reference's 4x4 CV_64F matrices (bottom row 0 0 0 1 stays exact under products and
// inverses), row-major.
#pragma once
#include <hip/hip_runtime.h>

#include <cfloat>
#include <cmath>

#include "../../include/aar.h"
#include "../host/se3.h"

namespace aar {

struct CamTab {
    double K[9];
    double k[AAR_MAX_DIST];
};

// ---------------------------------------------------------------------------------------------------------------------
// IPPE.  Contraction is off: the float error below is a chain of individually rounded operations (ippe.cpp:289-321), and the
// double part then rounds like the reference's scalar code as well.
// ---------------------------------------------------------------------------------------------------------------------
#pragma clang fp contract(off)

__device__ __forceinline__ void d_mat3mul(const double *A, const double *B, double *C) {
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int j = 0; j < 3; j++) C[i * 3 + j] = A[i * 3] * B[j] + A[i * 3 + 1] * B[3 + j] + A[i * 3 + 2] * B[6 + j];
}

// least-squares translation for a fixed rotation (ippe.cpp:347-425): [n 0 Sa; 0 n Sb; Sa Sb Sq] t = B
__device__ __forceinline__ void d_ippe_translation(float hf, const float *q, const double *R, double *t) {
    const float mx[4] = {-hf, hf, hf, -hf}, my[4] = {hf, hf, -hf, -hf};
    double Sa = 0, Sb = 0, Sq = 0, B0 = 0, B1 = 0, B2 = 0;
#pragma unroll
    for (int i = 0; i < 4; i++) {
        const double X = mx[i], Y = my[i], Z = 0.0;
        const double rx = R[0] * X + R[1] * Y + R[2] * Z, ry = R[3] * X + R[4] * Y + R[5] * Z, rz = R[6] * X + R[7] * Y + R[8] * Z;
        const double a = -(double)q[2 * i], b = -(double)q[2 * i + 1];
        Sa += a; Sb += b; Sq += a * a + b * b;
        const double bx = (double)q[2 * i] * rz - rx, by = (double)q[2 * i + 1] * rz - ry;
        B0 += bx; B1 += by; B2 += a * bx + b * by;
    }
    const double n = 4;
    const double dinv = 1.0 / (n * n * Sq - n * Sb * Sb - Sa * n * Sa);
    t[0] = dinv * ((n * Sq - Sb * Sb) * B0 + (Sa * Sb) * B1 + (-Sa * n) * B2);
    t[1] = dinv * ((Sb * Sa) * B0 + (n * Sq - Sa * Sa) * B1 + (-n * Sb) * B2);
    t[2] = dinv * ((-n * Sa) * B0 + (-n * Sb) * B1 + (n * n) * B2);
}

__device__ __forceinline__ float d_ippe_error(float hf, const float *q, const double *R, const double *t) {
    const float mx[4] = {-hf, hf, hf, -hf}, my[4] = {hf, hf, -hf, -hf};
    float err = 0;
#pragma unroll
    for (int i = 0; i < 4; i++) {
        const float px = (float)(R[0] * mx[i]) + (float)(R[1] * my[i]) + (float)(R[2] * 0.0f + t[0]);
        const float py = (float)(R[3] * mx[i]) + (float)(R[4] * my[i]) + (float)(R[5] * 0.0f + t[1]);
        const float pz = (float)(R[6] * mx[i]) + (float)(R[7] * my[i]) + (float)(R[8] * 0.0f + t[2]);
        const float dx = px / pz - q[2 * i], dy = py / pz - q[2 * i + 1];
        err = err + sqrtf(dx * dx + dy * dy);
    }
    return err;
}

// IPPERot2vec (ippe.cpp:323-345), cv::Rodrigues back to a matrix and the CV_32F conversion of getRTMatrix (:40-93)
//
// Guard (a departure from ippe.cpp, as in oracle/init_oracle.cpp): within delta0 = 1e-3 rad of pi the matrix -> vector -> matrix round
// trip is skipped and R is rounded to float as it stands.  IPPERot2vec takes w = acos((trace - 1) / 2) and the axis from
// w / (2 sin w) (R - R^T); with delta = pi - w the rounding of the trace (~4e-16) is an angle error of about pi * 4e-16 / delta^2, one
// float ulp at delta ~ 1e-4 and garbage (often the identity) below 1e-6, and an argument rounded below -1 is a NaN.
// IPPE_PI_GUARD_C0 = delta0^2 / 2 = 1 - cos(delta0): at delta0 the round trip's error, pi * 4e-16 / 1e-6 ~ 1.3e-9, is still 100 times below
// a float ulp (1.2e-7), so the stored floats do not jump at the seam, and R's own departure from a rotation is ~1e-15.  The test is on the
// trace, negated (a NaN or an argument below -1 takes the guard); no libm call decides it.
#define IPPE_PI_GUARD_C0 5e-7
__device__ __forceinline__ void d_store_pose(const double *R, const double *t, double *out) {
    const double ca = (R[0] + R[4] + R[8] - 1.0) / 2.0;
    double M[9];
    if (!(ca > -1.0 + IPPE_PI_GUARD_C0)) {
#pragma unroll
        for (int i = 0; i < 9; i++) M[i] = R[i];
    } else {
        const double w = acos(ca);
        double rv0 = 0, rv1 = 0, rv2 = 0;
        if (!(w < DBL_EPSILON)) {
            const double d = 1 / (2 * sin(w)) * w;
            rv0 = d * (R[7] - R[5]); rv1 = d * (R[2] - R[6]); rv2 = d * (R[3] - R[1]);
        }
        const double th = sqrt(rv0 * rv0 + rv1 * rv1 + rv2 * rv2);
        if (th < DBL_EPSILON) {
#pragma unroll
            for (int i = 0; i < 9; i++) M[i] = (i % 4 == 0) ? 1.0 : 0.0;
        } else {
            const double c = cos(th), s = sin(th), c1 = 1. - c, ith = 1. / th;
            const double x = rv0 * ith, y = rv1 * ith, z = rv2 * ith;
            M[0] = c + c1 * x * x;     M[1] = c1 * x * y - s * z; M[2] = c1 * x * z + s * y;
            M[3] = c1 * x * y + s * z; M[4] = c + c1 * y * y;     M[5] = c1 * y * z - s * x;
            M[6] = c1 * x * z - s * y; M[7] = c1 * y * z + s * x; M[8] = c + c1 * z * z;
        }
    }
#pragma unroll
    for (int i = 0; i < 3; i++) {
#pragma unroll
        for (int j = 0; j < 3; j++) out[i * 4 + j] = (double)(float)M[i * 3 + j];
        out[i * 4 + 3] = (double)(float)t[i];
    }
}

// cv::undistortPoints on the four corners uv of one detection: five fixed-point iterations of the inverse distortion model; normalised
// output q for IPPE (ippe.cpp:167), P = K output uvK for the data set (libs/multicam_mapper.cpp:554-578)
__device__ __forceinline__ void d_undistort4(const float *uv, const CamTab &cm, float *q, float *uvK) {
    const double *K = cm.K, *k = cm.k;
    const double ifx = 1.0 / K[0], ify = 1.0 / K[4];
#pragma unroll
    for (int c = 0; c < 4; c++) {
        double x = ((double)uv[2 * c] - K[2]) * ifx, y = ((double)uv[2 * c + 1] - K[5]) * ify;
        const double x0 = x, y0 = y;
#pragma unroll 1
        for (int it = 0; it < 5; it++) {
            const double r2 = x * x + y * y;
            const double icdist = (1.0 + ((k[7] * r2 + k[6]) * r2 + k[5]) * r2) / (1.0 + ((k[4] * r2 + k[1]) * r2 + k[0]) * r2);
            const double dx = 2.0 * k[2] * x * y + k[3] * (r2 + 2.0 * x * x) + k[8] * r2 + k[9] * r2 * r2;
            const double dy = k[2] * (r2 + 2.0 * y * y) + 2.0 * k[3] * x * y + k[10] * r2 + k[11] * r2 * r2;
            x = (x0 - dx) * icdist;
            y = (y0 - dy) * icdist;
        }
        q[2 * c] = (float)x;
        q[2 * c + 1] = (float)y;
        const double xx = K[0] * x + K[1] * y + K[2], yy = K[3] * x + K[4] * y + K[5], ww = 1.0 / (K[6] * x + K[7] * y + K[8]);
        uvK[2 * c] = (float)(xx * ww);
        uvK[2 * c + 1] = (float)(yy * ww);
    }
}

// the two float-rounded poses of the square with half side hf seen at the normalised corners q, the one with the smaller float
// reprojection error first (pose0 / e1), and the two errors
__device__ __forceinline__ void d_ippe_square(float hf, const float *q, double *pose0, double *pose1, float &e1, float &e2) {
    // homography of the square (-h,h),(h,h),(h,-h),(-h,-h) onto q, h22 = 1: unit square -> quadrilateral, composed with the
    // affine map of the marker frame (the closed form ippe.cpp:538-578 expands)
    double H[9];
    {
        const double h = (double)hf;
        const double x0 = q[0], y0 = q[1], x1 = q[2], y1 = q[3], x2 = q[4], y2 = q[5], x3 = q[6], y3 = q[7];
        const double sx = x0 - x1 + x2 - x3, sy = y0 - y1 + y2 - y3;
        const double dx1 = x1 - x2, dx2 = x3 - x2, dy1 = y1 - y2, dy2 = y3 - y2;
        const double den = dx1 * dy2 - dy1 * dx2;
        const double g = (sx * dy2 - sy * dx2) / den, kk = (dx1 * sy - dy1 * sx) / den;
        const double U[9] = {x1 - x0 + g * x1, x3 - x0 + kk * x3, x0, y1 - y0 + g * y1, y3 - y0 + kk * y3, y0, g, kk, 1.0};
        const double s = 1.0 / (2.0 * h);
        double Hn[9];
#pragma unroll
        for (int r = 0; r < 3; r++) {
            Hn[r * 3 + 0] = U[r * 3 + 0] * s;
            Hn[r * 3 + 1] = -U[r * 3 + 1] * s;
            Hn[r * 3 + 2] = 0.5 * (U[r * 3 + 0] + U[r * 3 + 1]) + U[r * 3 + 2];
        }
#pragma unroll
        for (int i = 0; i < 9; i++) H[i] = Hn[i] / Hn[8];
    }
    // the two rotations (ippe.cpp:427-536; IPPE paper, Algorithm 1)
    double Ra[9], Rb[9];
    {
        const double J0 = H[0] - H[6] * H[2], J1 = H[1] - H[7] * H[2], J2 = H[3] - H[6] * H[5], J3 = H[4] - H[7] * H[5];
        const double p = H[2], qq = H[5];
        const double s = sqrt(p * p + qq * qq + 1), t = sqrt(p * p + qq * qq);
        const double ct = 1 / s, st = sqrt(1 - 1 / (s * s));
        // guard (a departure from ippe.cpp, which divides 0 / 0 here): the centre maps exactly onto the principal point, Rv = I
        const double kx = t == 0 ? 0.0 : p / t, ky = t == 0 ? 0.0 : qq / t;
        const double Rv[9] = {(ct - 1) * kx * kx + 1, kx * ky * (ct - 1),     kx * st,
                              kx * ky * (ct - 1),     (ct - 1) * ky * ky + 1, ky * st,
                              -kx * st,               -ky * st,               (ct - 1) * (kx * kx + ky * ky) + 1};
        const double b00 = Rv[0] - p * Rv[6], b01 = Rv[1] - p * Rv[7], b10 = Rv[3] - qq * Rv[6], b11 = Rv[4] - qq * Rv[7];
        const double di = 1.0 / (b00 * b11 - b01 * b10);
        const double i00 = di * b11, i01 = -di * b01, i10 = -di * b10, i11 = di * b00;
        const double a00 = i00 * J0 + i01 * J2, a01 = i00 * J1 + i01 * J3;
        const double a10 = i10 * J0 + i11 * J2, a11 = i10 * J1 + i11 * J3;
        const double n00 = a00 * a00 + a01 * a01, n01 = a00 * a10 + a01 * a11, n11 = a10 * a10 + a11 * a11;
        const double gamma = sqrt(0.5 * (n00 + n11 + sqrt((n00 - n11) * (n00 - n11) + 4.0 * n01 * n01)));
        const double r00 = a00 / gamma, r01 = a01 / gamma, r10 = a10 / gamma, r11 = a11 / gamma;
        // guard (a departure from ippe.cpp): a column of A / gamma that is a unit vector leaves a radicand of about -1e-16, clamped at 0
        // (a NaN stays a NaN)
        const double g0 = -r00 * r00 - r10 * r10 + 1, g1 = -r01 * r01 - r11 * r11 + 1;
        const double b0 = sqrt(g0 < 0 ? 0.0 : g0);
        double b1 = sqrt(g1 < 0 ? 0.0 : g1);
        if (-r00 * r01 - r10 * r11 < 0) b1 = -b1;
        const double Qa[9] = {r00, r01, b1 * r10 - b0 * r11, r10, r11, b0 * r01 - b1 * r00, b0, b1, r00 * r11 - r01 * r10};
        const double Qb[9] = {r00, r01, b0 * r11 - b1 * r10, r10, r11, b1 * r00 - b0 * r01, -b0, -b1, r00 * r11 - r01 * r10};
        d_mat3mul(Rv, Qa, Ra);
        d_mat3mul(Rv, Qb, Rb);
    }
    double ta[3], tb[3];
    d_ippe_translation(hf, q, Ra, ta);
    d_ippe_translation(hf, q, Rb, tb);
    const float ea = d_ippe_error(hf, q, Ra, ta), eb = d_ippe_error(hf, q, Rb, tb);
    const bool a_first = ea < eb;
    d_store_pose(Ra, ta, a_first ? pose0 : pose1);
    d_store_pose(Rb, tb, a_first ? pose1 : pose0);
    e1 = a_first ? ea : eb;
    e2 = a_first ? eb : ea;
}

#pragma clang fp contract(fast)

// ---------------------------------------------------------------------------------------------------------------------
// 3x4 affine helpers
// ---------------------------------------------------------------------------------------------------------------------
struct Aff {
    double m[12];
};

__device__ __forceinline__ Aff aff_load(const double *__restrict__ p) {
    Aff a;
#pragma unroll
    for (int i = 0; i < 12; i++) a.m[i] = p[i];
    return a;
}
__device__ __forceinline__ void aff_store(double *__restrict__ p, const Aff &a) {
#pragma unroll
    for (int i = 0; i < 12; i++) p[i] = a.m[i];
}
__device__ __forceinline__ Aff aff_identity() {
    Aff a;
#pragma unroll
    for (int i = 0; i < 12; i++) a.m[i] = (i % 5 == 0) ? 1.0 : 0.0;
    return a;
}
// x * y, every element accumulated over k = 0..3 in order as a 4x4 cv::Mat product does
__device__ __forceinline__ Aff aff_mul(const Aff &x, const Aff &y) {
    Aff r;
#pragma unroll
    for (int i = 0; i < 3; i++) {
#pragma unroll
        for (int j = 0; j < 3; j++)
            r.m[i * 4 + j] = x.m[i * 4] * y.m[j] + x.m[i * 4 + 1] * y.m[4 + j] + x.m[i * 4 + 2] * y.m[8 + j];
        r.m[i * 4 + 3] = x.m[i * 4] * y.m[3] + x.m[i * 4 + 1] * y.m[7] + x.m[i * 4 + 2] * y.m[11] + x.m[i * 4 + 3];
    }
    return r;
}
// general inverse (cv::Mat::inv() of the 4x4): the poses are float-rounded, so R^T is NOT the inverse
__device__ __forceinline__ Aff aff_inv(const Aff &x) {
    const double a = x.m[0], b = x.m[1], c = x.m[2], d = x.m[4], e = x.m[5], f = x.m[6], g = x.m[8], h = x.m[9], i = x.m[10];
    const double c00 = e * i - f * h, c01 = f * g - d * i, c02 = d * h - e * g;
    const double idet = 1.0 / (a * c00 + b * c01 + c * c02);
    Aff r;
    r.m[0] = c00 * idet; r.m[1] = (c * h - b * i) * idet; r.m[2] = (b * f - c * e) * idet;
    r.m[4] = c01 * idet; r.m[5] = (a * i - c * g) * idet; r.m[6] = (c * d - a * f) * idet;
    r.m[8] = c02 * idet; r.m[9] = (b * g - a * h) * idet; r.m[10] = (a * e - b * d) * idet;
#pragma unroll
    for (int k = 0; k < 3; k++) r.m[k * 4 + 3] = -(r.m[k * 4] * x.m[3] + r.m[k * 4 + 1] * x.m[7] + r.m[k * 4 + 2] * x.m[11]);
    return r;
}

// j-side record of the vote: T2_inv (12) followed by T1_inv * corners (3 x 4, column c = corner c)
__device__ __forceinline__ void store_jside(double *__restrict__ bj, const Aff &T1inv, const Aff &T2inv, double h) {
    aff_store(bj, T2inv);
    const double px[4] = {-h, h, h, -h}, py[4] = {h, h, -h, -h};
#pragma unroll
    for (int r = 0; r < 3; r++)
#pragma unroll
        for (int c = 0; c < 4; c++) bj[12 + r * 4 + c] = T1inv.m[r * 4] * px[c] + T1inv.m[r * 4 + 1] * py[c] + T1inv.m[r * 4 + 3];
}

// fill_transformation_set (libs/initializer.cpp:73-93): the object pose candidate (root marker -> root camera) through one detection with
// marker -> camera pose T_mc, its camera's and marker's to-root transforms, and the candidate's j-side record
__device__ __forceinline__ void object_cand(const Aff &T_mc, const Aff &T_cr, const Aff &T_mr, double h, double *__restrict__ Tc,
                                            double *__restrict__ bj) {
    const Aff T_rm = aff_inv(T_mr), T_rc = aff_inv(T_cr), T_cm = aff_inv(T_mc);
    aff_store(Tc, aff_mul(aff_mul(T_cr, T_mc), T_rm));
    store_jside(bj, aff_mul(T_mr, T_cm), T_rc, h);
}

// sqrt for the vote: v_rsq_f64 seed (~2^-26) + one coupled Goldschmidt step + one residual correction = full double accuracy
// (<= 1 ulp) in 8 instructions, without the range scaling of the library sqrt (the arguments are squared distances of
// metre-sized scenes, nowhere near the denormals); an exact zero stays an exact zero.
__device__ __forceinline__ double vote_sqrt(double q) {
    const double y = __builtin_amdgcn_rsq(q);
    double g = q * y, h = 0.5 * y;
    const double r = fma(-h, g, 0.5);
    g = fma(g, r, g);
    h = fma(h, r, h);
    const double d = fma(-g, g, q);
    g = fma(d, h, g);
    return q == 0.0 ? 0.0 : g;   // (a NaN argument stays NaN: such a candidate must never win the vote)
}

// one (i, j) term of find_best_transformation: sum over the four corners of |p - T2inv_j T_i T1inv_j p|, T = T_i, b = j's record
__device__ __forceinline__ double vote_term(const double *T, const double *__restrict__ b, const double *px, const double *py) {
    double s = 0;
#pragma unroll
    for (int c = 0; c < 4; c++) {
        const double ax = b[12 + c], ay = b[16 + c], az = b[20 + c];
        // three-term rows as FMA chains ending in the translation (one instruction per product, none for the additions)
        const double rx = fma(T[0], ax, fma(T[1], ay, fma(T[2], az, T[3])));
        const double ry = fma(T[4], ax, fma(T[5], ay, fma(T[6], az, T[7])));
        const double rz = fma(T[8], ax, fma(T[9], ay, fma(T[10], az, T[11])));
        const double dx = px[c] - fma(b[0], rx, fma(b[1], ry, fma(b[2], rz, b[3])));
        const double dy = py[c] - fma(b[4], rx, fma(b[5], ry, fma(b[6], rz, b[7])));
        const double dz = -fma(b[8], rx, fma(b[9], ry, fma(b[10], rz, b[11])));
        s += vote_sqrt(fma(dx, dx, fma(dy, dy, dz * dz)));
    }
    return s;
}

// transformation_mat2vec (libs/multicam_mapper.cpp:475-486) of a 3x4: host/se3.h's rodrigues_mat2vec, compiled for the device
__device__ inline void aff_to_pose6(const double *m, double v[6]) {
    double R[9];
#pragma unroll
    for (int i = 0; i < 3; i++) {
#pragma unroll
        for (int j = 0; j < 3; j++) R[i * 3 + j] = m[i * 4 + j];
        v[3 + i] = m[i * 4 + 3];
    }
    rodrigues_mat2vec(R, v);
}

}  // namespace aar
