// The second-difference term of the constant-velocity prior and its Jacobians, shared by the smoothed tracker
// (smooth_cv_kernels.hip) and the sigma fit under that prior (smooth_cv_fit_kernels.hip).  fp64, registers only; see smooth_cv_kernels.hip
// for the derivation.
#pragma once
#include "geom.hpp"
#include "so3.hpp"

namespace aar {

// Exp(x) and J_r(x) = I - A [x]x + B [x]x^2 (row-major)
__device__ __forceinline__ void so3_exp_jr(const double *x, double *R, double *Jr) {
    const double t2 = x[0] * x[0] + x[1] * x[1] + x[2] * x[2], th = sqrt(t2);
    double a, A, B;   // sin / th, (1 - cos) / th^2, (th - sin) / th^3
    if (th < 1e-2) {
        a = 1.0 - t2 * (1.0 / 6.0) + t2 * t2 * (1.0 / 120.0);
        A = 0.5 - t2 * (1.0 / 24.0) + t2 * t2 * (1.0 / 720.0);
        B = (1.0 / 6.0) - t2 * (1.0 / 120.0) + t2 * t2 * (1.0 / 5040.0);
    } else {
        double s, c;
        sincos(th, &s, &c);
        const double it2 = 1.0 / t2;
        a = s / th;
        A = (1.0 - c) * it2;
        B = (th - s) * it2 / th;
    }
    const double wx = x[0], wy = x[1], wz = x[2];
    // [x]x^2 = x x^T - |x|^2 I
    const double d0 = wx * wx - t2, d1 = wy * wy - t2, d2 = wz * wz - t2, xy = wx * wy, xz = wx * wz, yz = wy * wz;
    R[0] = 1.0 + A * d0;      R[1] = -a * wz + A * xy;  R[2] = a * wy + A * xz;
    R[3] = a * wz + A * xy;   R[4] = 1.0 + A * d1;      R[5] = -a * wx + A * yz;
    R[6] = -a * wy + A * xz;  R[7] = a * wx + A * yz;   R[8] = 1.0 + A * d2;
    Jr[0] = 1.0 + B * d0;     Jr[1] = A * wz + B * xy;  Jr[2] = -A * wy + B * xz;
    Jr[3] = -A * wz + B * xy; Jr[4] = 1.0 + B * d1;     Jr[5] = A * wx + B * yz;
    Jr[6] = A * wy + B * xz;  Jr[7] = -A * wx + B * yz; Jr[8] = 1.0 + B * d2;
}

__device__ __forceinline__ void mm3(const double *X, const double *Y, double *Z) {    // Z = X Y
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int j = 0; j < 3; j++) Z[3 * i + j] = X[3 * i] * Y[j] + X[3 * i + 1] * Y[3 + j] + X[3 * i + 2] * Y[6 + j];
}
__device__ __forceinline__ void mtm3(const double *X, const double *Y, double *Z) {   // Z = X^T Y
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int j = 0; j < 3; j++) Z[3 * i + j] = X[i] * Y[j] + X[3 + i] * Y[3 + j] + X[6 + i] * Y[6 + j];
}
__device__ __forceinline__ void mmt3(const double *X, const double *Y, double *Z) {   // Z = X Y^T
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int j = 0; j < 3; j++) Z[3 * i + j] = X[3 * i] * Y[3 * j] + X[3 * i + 1] * Y[3 * j + 1] + X[3 * i + 2] * Y[3 * j + 2];
}

// e (phi, e_t) of the term over the entity rows of frames f - 1, f, f + 1; WITH_J: M_p, M_c, M_n
template <bool WITH_J>
__device__ __forceinline__ void cv_term(const double *rp, const double *rc, const double *rn, double r, double phi[3], double et[3], double Mp[9],
                                        double Mc[9], double Mn[9]) {
    double P[9], A[9], psi[3], thp;
    mtm3(rp, rc, P);   // R_{f-1}^T R_f
    mtm3(rc, rn, A);   // R_f^T R_{f+1}
    so3_log(P, psi, thp);
    const double rv[3] = {r * psi[0], r * psi[1], r * psi[2]};
    double dR[9], Jrr[9], Q[9], th;
    so3_exp_jr(rv, dR, Jrr);
    mtm3(dR, A, Q);
    so3_log(Q, phi, th);
#pragma unroll
    for (int i = 0; i < 3; i++) et[i] = rn[9 + i] - rc[9 + i] - r * (rc[9 + i] - rp[9 + i]);
    if (WITH_J) {
        double Ji[9], Jpi[9], X[9], Y[9], B[9], T[9], S[9], U[9];
        so3_jr_inv(phi, th, Ji);
        so3_jr_inv(psi, thp, Jpi);
        mm3(Jrr, Jpi, X);
        mtm3(Q, X, Y);
        mm3(Ji, Y, B);
        const double *Jp = rp + 12, *Jc = rc + 12, *Jn = rn + 12;
        mmt3(Ji, Jn, Mn);
        mtm3(rn, Jc, T);    // R_{f+1}^T J_l(w_f)
        mm3(Ji, T, S);
        mmt3(B, Jc, U);     // B J_l(w_f)^T
#pragma unroll
        for (int i = 0; i < 9; i++) Mc[i] = -S[i] - r * U[i];
        mtm3(rc, Jp, T);    // R_f^T J_l(w_{f-1})
        mm3(B, T, S);
#pragma unroll
        for (int i = 0; i < 9; i++) Mp[i] = r * S[i];
    }
}

}  // namespace aar
