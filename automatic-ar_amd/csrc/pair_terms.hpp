// The between factor of two consecutive frame poses and its Jacobians, shared by the smoothed tracker
// (smooth_kernels.hip) and the live tracker (live_kernels.hip).  fp64, registers only; see smooth_kernels.hip for the derivation.
#pragma once
#include "geom.hpp"
#include "so3.hpp"

namespace aar {

__device__ __forceinline__ void ld6(const double *p, double *v) {
#pragma unroll
    for (int i = 0; i < 6; i++) v[i] = p[i];
}

// e (phi, e_t) of the pair (a, b) from the entity rows of the two poses; WITH_J: M_a, M_b
template <bool WITH_J>
__device__ __forceinline__ void pair_terms(const double *ra, const double *rb, const double *rel, double phi[3], double et[3], double Ma[9], double Mb[9]) {
    double P[9];   // R_a^T R_b
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int j = 0; j < 3; j++) P[3 * i + j] = ra[i] * rb[j] + ra[3 + i] * rb[3 + j] + ra[6 + i] * rb[6 + j];
    double Q[9];
    double dt[3] = {0.0, 0.0, 0.0};
    if (rel) {
        double rr[ENT_STRIDE];
        make_ent_row(rel, rr);
#pragma unroll
        for (int i = 0; i < 3; i++)
#pragma unroll
            for (int j = 0; j < 3; j++) Q[3 * i + j] = rr[i] * P[j] + rr[3 + i] * P[3 + j] + rr[6 + i] * P[6 + j];
        dt[0] = rel[3]; dt[1] = rel[4]; dt[2] = rel[5];
    } else {
#pragma unroll
        for (int i = 0; i < 9; i++) Q[i] = P[i];
    }
    double th;
    so3_log(Q, phi, th);
#pragma unroll
    for (int i = 0; i < 3; i++) et[i] = rb[9 + i] - ra[9 + i] - dt[i];
    if (WITH_J) {
        double Ji[9];
        so3_jr_inv(phi, th, Ji);
        const double *Ja = ra + 12, *Jb = rb + 12;
        double T[9];   // R_b^T J_l(w_a)
#pragma unroll
        for (int k = 0; k < 3; k++)
#pragma unroll
            for (int j = 0; j < 3; j++) T[3 * k + j] = rb[k] * Ja[j] + rb[3 + k] * Ja[3 + j] + rb[6 + k] * Ja[6 + j];
#pragma unroll
        for (int i = 0; i < 3; i++)
#pragma unroll
            for (int j = 0; j < 3; j++) {
                Mb[3 * i + j] = Ji[3 * i] * Jb[3 * j] + Ji[3 * i + 1] * Jb[3 * j + 1] + Ji[3 * i + 2] * Jb[3 * j + 2];
                Ma[3 * i + j] = -(Ji[3 * i] * T[j] + Ji[3 * i + 1] * T[3 + j] + Ji[3 * i + 2] * T[6 + j]);
            }
    }
}

}  // namespace aar
