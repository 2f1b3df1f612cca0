// 12x12 blocks with one wavefront per block: lane i < 12 holds row i of a block in twelve registers (lanes 12..63
// repeat lane 11 and store nothing); row p of another operand reaches every lane through v_readlane, so a product is 144 broadcasts and
// 144 fma per lane, every sum in ascending p.  Transposes cost nothing: a lane loads column i instead of row i.
// Shared by the constant-velocity solve (smooth_cv_kernels.hip) and its selected inverse (smooth_cv_cov_kernels.hip).
#pragma once
#include <hip/hip_runtime.h>
#include "kernels.h"

namespace aar {

namespace {

__device__ __forceinline__ double bc(double v, int l) {
    return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(v), l), __builtin_amdgcn_readlane(__double2loint(v), l));
}
__device__ __forceinline__ void ld_row(const double *M, int i, double *r) {
#pragma unroll
    for (int j = 0; j < 12; j++) r[j] = M[12 * i + j];
}
__device__ __forceinline__ void ld_col(const double *M, int i, double *r) {
#pragma unroll
    for (int p = 0; p < 12; p++) r[p] = M[12 * p + i];
}
__device__ __forceinline__ void st_row(double *M, int lane, const double *r) {
    if (lane < 12) {
#pragma unroll
        for (int j = 0; j < 12; j++) M[12 * lane + j] = r[j];
    }
}
// C (+)= sg * A B: this lane's row of A times the rows of B held by lanes 0..11
template <bool ACC>
__device__ __forceinline__ void row_mm(const double *A, const double *B, double sg, double *C) {
    double t[12];
#pragma unroll
    for (int j = 0; j < 12; j++) t[j] = 0.0;
#pragma unroll
    for (int p = 0; p < 12; p++)
#pragma unroll
        for (int j = 0; j < 12; j++) t[j] = fma(A[p], bc(B[j], p), t[j]);
#pragma unroll
    for (int j = 0; j < 12; j++) C[j] = ACC ? C[j] + sg * t[j] : sg * t[j];
}
// sum_p A[p] x_p, x_p held by lane p
__device__ __forceinline__ double row_mv(const double *A, double x) {
    double t = 0.0;
#pragma unroll
    for (int p = 0; p < 12; p++) t = fma(A[p], bc(x, p), t);
    return t;
}
// in-place Gauss-Jordan inverse of a positive definite block, no pivoting (the pivots are those of its Cholesky factor, squared);
// false: a pivot was not positive
__device__ __forceinline__ bool row_inverse(int ri, double *a) {
    bool ok = true;
#pragma unroll
    for (int k = 0; k < 12; k++) {
        double pr[12];
#pragma unroll
        for (int j = 0; j < 12; j++) pr[j] = bc(a[j], k);
        const double p = pr[k];
        ok = ok && p > 0.0;
        const double ip = 1.0 / p, f = a[k];
        const bool own = ri == k;
#pragma unroll
        for (int j = 0; j < 12; j++) {
            const double s = pr[j] * ip;
            if (j != k) a[j] = own ? s : fma(-f, s, a[j]);
        }
        a[k] = own ? ip : -f * ip;
    }
    return ok;
}

__device__ __forceinline__ int wave_of_block() { return __builtin_amdgcn_readfirstlane(threadIdx.x >> 6); }

inline int cv_evens(int K, int stride) { return (K + 2 * stride - 1) / (2 * stride); }
// the levels that get a launch of their own: strides 1, 2, ... while a level has more than SMOOTH_CV_T eliminating supernodes
inline int cv_own_levels(int K) {
    int n = 0;
    for (int s = 1; s < K && cv_evens(K, s) > SMOOTH_CV_T; s *= 2) n++;
    return n;
}

}  // namespace

}  // namespace aar
