// Pose covariance of smoothed tracks: the diagonal and lag-one 6x6 blocks of H^-1 for the block-tridiagonal H of
// aar_track_smooth, from what the block cyclic reduction of smooth_kernels.hip leaves behind after one solve at mu = 0:
//   Dinv[i]  the inverse pivot of every eliminated node i
//   Ls[i]    the coupling from its left neighbour p = i - s (rows p, columns i) at the stride s it was eliminated at
//   Uw[i]    its coupling to its right neighbour q = i + s (rows i, columns q); stale when q >= F, and then not read
//   Dw[0]    the root pivot
// One pass back down the elimination tree (the shape of cr_backsub, with 6x6 blocks where that carries 6-vectors).  Eliminating i meant
//   x_i = Dinv[i] b_i - G_p x_p - G_q x_q,   G_p = Dinv[i] Ls[i]^T,  G_q = Dinv[i] Uw[i]
// so with S[n] = Sigma_nn and R[n] = Sigma between n and the next active node on its right at the current stride:
//   root      S[0] = Dw[0]^-1
//   node i    Sigma_ip = -(G_p S[p] + G_q R[p]^T),  Sigma_iq = -(G_p R[p] + G_q S[q]),  S[i] = Dinv[i] - Sigma_ip G_p^T - Sigma_iq G_q^T
//             R[i] = Sigma_iq,  R[p] = Sigma_ip^T                                        (the q terms absent when q >= F)
// At one level node i is the only reader of R[p] and the only writer of R[p], R[i] and S[i]; S[p] and S[q] belong to coarser levels.  So the
// pass is in place with one owner per store: no atomics, a fixed order, the same bits from call to call.  S[i] is computed on its lower
// triangle and mirrored: the diagonal blocks are symmetric to the bit.  After stride 1, S = frame_cov and R[0 .. F-2] = lag_cov.
//
// Launches mirror launch_smooth_solve upside down: ONE workgroup runs the root and every level the solve's tail ran, then one launch per
// finer level, one thread per node.  Plain fp64 loads and stores; no LDS.
#include <algorithm>
#include "geom.hpp"
#include "kernels.h"

namespace aar {

namespace {

struct SelArgs {
    const double *Dg, *Dw, *Uw, *Dinv, *Ls;   // H's diagonal blocks and what the reduction left (SmoothWork)
    double *S, *R;                       // [F][36] each
    int32_t *flag;
    int F;
};

__device__ __forceinline__ void sc_ld36(const double *p, double *m) {
#pragma unroll
    for (int i = 0; i < 36; i++) m[i] = p[i];
}

// Dw[0] is the Schur complement of H onto frame 0, formed by subtracting from H_00: it carries a rounding error of the order eps |H_00|.  A
// pivot of its LDL^T that is not above SELINV_ROOT_TOL times the largest diagonal entry of H_00 cannot be told from zero and counts as
// non-positive (the prior alone: the exact root is singular, the computed one is rounding noise of either sign).
constexpr double SELINV_ROOT_TOL = 64.0 * 2.220446049250313e-16;

__device__ __forceinline__ void sc_root(const SelArgs &a) {
    double m[6][6], l[6][6], I[36];
    double top = 0.0;
#pragma unroll
    for (int i = 0; i < 6; i++) {
        top = fmax(top, a.Dg[7 * i]);
#pragma unroll
        for (int j = 0; j < 6; j++) m[i][j] = l[i][j] = a.Dw[6 * i + j];
    }
    bool ok = true;
#pragma unroll
    for (int p = 0; p < 6; p++) {
        const double d = l[p][p];
        if (!(d > SELINV_ROOT_TOL * top)) ok = false;
        const double di = 1.0 / (ok ? d : 1.0);
#pragma unroll
        for (int q = p + 1; q < 6; q++)
#pragma unroll
            for (int r = p + 1; r <= q; r++) l[q][r] = fma(-l[q][p] * di, l[r][p], l[q][r]);
    }
    if (!spd6_inverse(m, I)) ok = false;
    if (!ok) a.flag[0] = 1;
#pragma unroll
    for (int i = 0; i < 36; i++) a.S[i] = I[i];
}

// eliminated node i (an odd multiple of s)
__device__ __forceinline__ void sc_node(const SelArgs &a, int i, int s) {
    const int p = i - s, q = i + s;
    const bool hq = q < a.F;
    const double *di = a.Dinv + 36 * (size_t)i;
    double Gp[36], Gq[36];
    {
        double I[36], M[36];
        sc_ld36(di, I);
        sc_ld36(a.Ls + 36 * (size_t)i, M);
#pragma unroll
        for (int r = 0; r < 6; r++)
#pragma unroll
            for (int c = 0; c < 6; c++) {
                double t = 0.0;
#pragma unroll
                for (int k = 0; k < 6; k++) t = fma(I[6 * r + k], M[6 * c + k], t);
                Gp[6 * r + c] = t;
            }
        if (hq) {
            sc_ld36(a.Uw + 36 * (size_t)i, M);
#pragma unroll
            for (int r = 0; r < 6; r++)
#pragma unroll
                for (int c = 0; c < 6; c++) {
                    double t = 0.0;
#pragma unroll
                    for (int k = 0; k < 6; k++) t = fma(I[6 * r + k], M[6 * k + c], t);
                    Gq[6 * r + c] = t;
                }
        }
    }
    // A = G_p S[p] + G_q R[p]^T (= -Sigma_ip) and B = G_p R[p] + G_q S[q] (= -Sigma_iq), the neighbours' blocks streamed from memory
    const double *sp = a.S + 36 * (size_t)p, *sq = a.S + 36 * (size_t)q, *rin = a.R + 36 * (size_t)p;
    double A[36], B[36];
#pragma unroll
    for (int c = 0; c < 6; c++) {
        double x[6];
#pragma unroll
        for (int k = 0; k < 6; k++) x[k] = sp[6 * k + c];
#pragma unroll
        for (int r = 0; r < 6; r++) {
            double t = 0.0;
#pragma unroll
            for (int k = 0; k < 6; k++) t = fma(Gp[6 * r + k], x[k], t);
            A[6 * r + c] = t;
        }
    }
    if (hq) {
#pragma unroll
        for (int c = 0; c < 6; c++) {
            double x[6], y[6], z[6];
#pragma unroll
            for (int k = 0; k < 6; k++) { x[k] = rin[6 * c + k]; y[k] = rin[6 * k + c]; z[k] = sq[6 * k + c]; }
#pragma unroll
            for (int r = 0; r < 6; r++) {
                double t = A[6 * r + c], u = 0.0;
#pragma unroll
                for (int k = 0; k < 6; k++) t = fma(Gq[6 * r + k], x[k], t);
#pragma unroll
                for (int k = 0; k < 6; k++) u = fma(Gp[6 * r + k], y[k], u);
#pragma unroll
                for (int k = 0; k < 6; k++) u = fma(Gq[6 * r + k], z[k], u);
                A[6 * r + c] = t;
                B[6 * r + c] = u;
            }
        }
    }
    // S[i] = Dinv[i] + A G_p^T + B G_q^T on the lower triangle, mirrored
    double *si = a.S + 36 * (size_t)i, *ri = a.R + 36 * (size_t)i, *rp = a.R + 36 * (size_t)p;
#pragma unroll
    for (int r = 0; r < 6; r++)
#pragma unroll
        for (int c = 0; c <= r; c++) {
            double t = di[6 * r + c];
#pragma unroll
            for (int k = 0; k < 6; k++) t = fma(A[6 * r + k], Gp[6 * c + k], t);
            if (hq) {
#pragma unroll
                for (int k = 0; k < 6; k++) t = fma(B[6 * r + k], Gq[6 * c + k], t);
            }
            si[6 * r + c] = t;
            if (c != r) si[6 * c + r] = t;
        }
    // (every read of R[p] lies before this point)
#pragma unroll
    for (int r = 0; r < 6; r++)
#pragma unroll
        for (int c = 0; c < 6; c++) {
            rp[6 * c + r] = -A[6 * r + c];
            if (hq) ri[6 * r + c] = -B[6 * r + c];
        }
}

__global__ void __launch_bounds__(64) k_selinv_level(const SelArgs a, int s) {
    const int64_t i = (int64_t)(blockIdx.x * 64 + threadIdx.x) * 2 * s + s;
    if (i < a.F) sc_node(a, (int)i, s);
}

// one workgroup: the root, then every level from the top stride down to s0, separated by workgroup barriers
__global__ void __launch_bounds__(SMOOTH_TAIL) k_selinv_tail(const SelArgs a, int s0) {
    const int t = threadIdx.x, F = a.F;
    if (t == 0) sc_root(a);
    __syncthreads();
    int s = 1;
    while (2 * (int64_t)s < F) s *= 2;
    if (F < 2) return;
    for (; s >= s0; s /= 2) {
        for (int64_t i = (int64_t)t * 2 * s + s; i < F; i += (int64_t)SMOOTH_TAIL * 2 * s) sc_node(a, (int)i, s);
        __syncthreads();
    }
}

}  // namespace

// after launch_smooth_solve(w, F, 0.0, st) on the same stream: S [F][36] = (H^-1)_ff, R [F][36] with R[f] = (H^-1)_{f,f+1} for f < F - 1;
// a root pivot that is not positive beyond its rounding level raises w.flag.  Returns its launches.
int launch_smooth_selinv(const SmoothWork &w, int F, double *S, double *R, hipStream_t st) {
    if (F == 0) return 0;
    SelArgs a;
    a.Dg = w.Dg; a.Dw = w.Dw; a.Uw = w.Uw; a.Dinv = w.Dinv; a.Ls = w.Ls; a.S = S; a.R = R; a.flag = w.flag; a.F = F;
    auto evens = [&](int stride) { return (F + 2 * stride - 1) / (2 * stride); };
    int s = 1;
    while (s < F && evens(s) > SMOOTH_TAIL) s *= 2;   // the stride launch_smooth_solve's tail started at
    hipLaunchKernelGGL(k_selinv_tail, dim3(1), dim3(SMOOTH_TAIL), 0, st, a, s);
    int launches = 1;
    for (s /= 2; s >= 1; s /= 2) {
        hipLaunchKernelGGL(k_selinv_level, dim3((evens(s) + 63) / 64), dim3(64), 0, st, a, s);
        launches++;
    }
    return launches;
}

}  // namespace aar
