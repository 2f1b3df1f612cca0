// Pose covariance of constant-velocity smoothed tracks: the diagonal, lag-one and lag-two 6x6 blocks of H^-1 for the
// block-pentadiagonal H of aar_track_smooth under AAR_SMOOTH_MODEL_CONSTANT_VELOCITY, from what the supernode cyclic reduction of
// smooth_cv_kernels.hip leaves behind after one solve at mu = 0:
//   Dinv[i]  the inverse pivot of every eliminated supernode i (12x12)
//   Ls[i]    the coupling from its left neighbour p = i - s (rows p, columns i) at the stride s it was eliminated at
//   Uw[i]    its coupling to its right neighbour q = i + s (rows i, columns q); stale when q >= K, and then not read
//   Dw[0]    the root pivot
// One pass back down the elimination tree, section 28's recursion on 12x12 blocks.  Eliminating i meant
//   x_i = Dinv[i] b_i - G_p x_p - G_q x_q,   G_p = Dinv[i] Ls[i]^T,  G_q = Dinv[i] Uw[i]
// so with S[n] = Sigma_nn and R[n] = Sigma between n and the next active supernode on its right at the current stride:
//   root      S[0] = Dw[0]^-1
//   node i    Sigma_ip = -(G_p S[p] + G_q R[p]^T),  Sigma_iq = -(G_p R[p] + G_q S[q]),  S[i] = Dinv[i] - Sigma_ip G_p^T - Sigma_iq G_q^T
//             R[i] = Sigma_iq,  R[p] = Sigma_ip^T                                        (the q terms absent when q >= K)
//
// One wavefront per supernode in the row layout of cv_rows.hpp.  Lane i reads entries of R[p] that other lanes of the same wavefront store
// as the new R[p]: R therefore PING-PONGS between two arrays by level (stride 2^e reads R[(e + 1) & 1] and writes R[e & 1]).  Every active
// supernode with a right neighbour has its R rewritten at every level -- an odd multiple i of s writes R[i] (when q < K), an even multiple p
// is written by i = p + s (when that is below K) -- so the array a level reads holds exactly what the level before wrote, and stride 1
// ends in R[0].  S[i] has node i as its only writer and S[p], S[q] belong to coarser levels.  One owner per store, no atomics, a fixed
// order: the same bits from call to call.  S[i] is formed in full rows and its upper triangle replaced by the lower one.
//
// After stride 1, supernode k = frames (2k, 2k + 1):
//   frame_cov[2k], frame_cov[2k+1]   the two diagonal 6x6 blocks of S[k]
//   lag_cov[2k]    = S[k][0:6, 6:12]      lag_cov[2k+1]  = R[k][6:12, 0:6]
//   lag2_cov[2k]   = R[k][0:6, 0:6]       lag2_cov[2k+1] = R[k][6:12, 6:12]            (R[k][0:6, 6:12], lag three, is dropped)
//
// Launches mirror launch_smooth_cv_solve upside down: ONE workgroup of four wavefronts runs the root and every level k_cv_tail ran, then
// one launch per finer level, then the unpacking.  Plain fp64 loads and stores; no LDS.
#include <algorithm>
#include "cv_rows.hpp"
#include "kernels.h"

namespace aar {

namespace {

struct CvSelArgs {
    const double *Dg, *Dw, *Uw, *Dinv, *Ls;   // H's diagonal blocks [F][36] and what the reduction left [K][144] (SmoothCvWork)
    double *S, *R[2];                         // [K][144] each
    int32_t *flag;
    int F, K;
};

// section 28's rule on the supernode: Dw[0] is the Schur complement of H onto frames 0 and 1, formed by subtracting from their blocks, so it
// carries a rounding error of the order eps |H_00|, eps |H_11|.  A pivot that is not above CV_ROOT_TOL times the largest diagonal entry of
// the live rows of supernode 0 of H cannot be told from zero and counts as non-positive.
constexpr double CV_ROOT_TOL = 64.0 * 2.220446049250313e-16;

// C += A B^T: this lane's row of A against row j of B, held by lane j
__device__ __forceinline__ void row_mmt_acc(const double *A, const double *B, double *C) {
    double t[12];
#pragma unroll
    for (int j = 0; j < 12; j++) t[j] = 0.0;
#pragma unroll
    for (int p = 0; p < 12; p++)
#pragma unroll
        for (int j = 0; j < 12; j++) t[j] = fma(A[p], bc(B[p], j), t[j]);
#pragma unroll
    for (int j = 0; j < 12; j++) C[j] += t[j];
}

// the upper triangle from the lower one: entry (i, j), j > i, becomes lane j's entry (j, i)
__device__ __forceinline__ void row_mirror(int ri, double *a) {
#pragma unroll
    for (int i = 0; i < 11; i++)
#pragma unroll
        for (int j = i + 1; j < 12; j++) {
            const double t = bc(a[i], j);
            if (ri == i) a[j] = t;
        }
}

__device__ __forceinline__ void cs_root(const CvSelArgs &a, int lane) {
    const int ri = lane < 12 ? lane : 11;
    const int live = a.F > 1 ? 12 : 6;   // F = 1: rows 6..11 are the padded identity
    double top = 0.0;
    for (int i = 0; i < live; i++) top = fmax(top, a.Dg[36 * (size_t)(i / 6) + 7 * (i % 6)]);
    const double tol = CV_ROOT_TOL * top;
    double I[12];
    ld_row(a.Dw, ri, I);
    bool ok = true;
    // row_inverse with the pivot rule on the live rows
#pragma unroll
    for (int k = 0; k < 12; k++) {
        double pr[12];
#pragma unroll
        for (int j = 0; j < 12; j++) pr[j] = bc(I[j], k);
        const double p = pr[k];
        ok = ok && (k < live ? p > tol : p > 0.0);
        const double ip = 1.0 / p, f = I[k];
        const bool own = ri == k;
#pragma unroll
        for (int j = 0; j < 12; j++) {
            const double s = pr[j] * ip;
            if (j != k) I[j] = own ? s : fma(-f, s, I[j]);
        }
        I[k] = own ? ip : -f * ip;
    }
    row_mirror(ri, I);
    st_row(a.S, lane, I);
    if (!ok && lane == 0) a.flag[0] = 1;
}

// eliminated supernode i (an odd multiple of s = 2^e)
__device__ __forceinline__ void cs_node(const CvSelArgs &a, int i, int s, int e, int lane) {
    const int ri = lane < 12 ? lane : 11, p = i - s, q = i + s;
    const bool hq = q < a.K;
    const double *rin = a.R[(e + 1) & 1] + 144 * (size_t)p;
    double *rout = a.R[e & 1];
    double I[12], M[12], Gp[12], Gq[12], A[12], B[12];
    ld_row(a.Dinv + 144 * (size_t)i, ri, I);
    ld_col(a.Ls + 144 * (size_t)i, ri, M);
    row_mm<false>(I, M, 1.0, Gp);
    // A = G_p S[p] + G_q R[p]^T (= -Sigma_ip) and B = G_p R[p] + G_q S[q] (= -Sigma_iq), the neighbours' blocks streamed from memory
    ld_row(a.S + 144 * (size_t)p, ri, M);
    row_mm<false>(Gp, M, 1.0, A);
    if (hq) {
        ld_row(a.Uw + 144 * (size_t)i, ri, M);
        row_mm<false>(I, M, 1.0, Gq);
        ld_col(rin, ri, M);
        row_mm<true>(Gq, M, 1.0, A);
        ld_row(rin, ri, M);
        row_mm<false>(Gp, M, 1.0, B);
        ld_row(a.S + 144 * (size_t)q, ri, M);
        row_mm<true>(Gq, M, 1.0, B);
    }
    // S[i] = Dinv[i] + A G_p^T + B G_q^T, the lower triangle mirrored
    row_mmt_acc(A, Gp, I);
    if (hq) row_mmt_acc(B, Gq, I);
    row_mirror(ri, I);
    st_row(a.S + 144 * (size_t)i, lane, I);
    if (lane < 12) {
        double *rp = rout + 144 * (size_t)p, *rn = rout + 144 * (size_t)i;
#pragma unroll
        for (int j = 0; j < 12; j++) {
            rp[12 * j + lane] = -A[j];   // R[p] = Sigma_ip^T: this lane's row is its column
            if (hq) rn[12 * lane + j] = -B[j];
        }
    }
}

__global__ void __launch_bounds__(256) k_cv_sel_level(const CvSelArgs a, int s, int e) {
    const int64_t i = (int64_t)(blockIdx.x * 4 + wave_of_block()) * 2 * s + s;
    if (i < a.K) cs_node(a, (int)i, s, e, threadIdx.x & 63);
}

// one workgroup of four wavefronts: the root, then every level from the top stride down to s0.  A wavefront takes the supernodes
// wv, wv + 4, ... of a level; the barriers stand BETWEEN the levels and the level loop runs on K and s0 alone, as in k_cv_tail.
__global__ void __launch_bounds__(256) k_cv_sel_tail(const CvSelArgs a, int s0) {
    const int lane = threadIdx.x & 63, wv = wave_of_block(), K = a.K;
    if (wv == 0) cs_root(a, lane);
    __syncthreads();
    int s = 1, e = 0;
    while (2 * (int64_t)s < K) { s *= 2; e++; }
    for (; s >= s0; s /= 2, e--) {
        for (int64_t i = (int64_t)wv * 2 * s + s; i < K; i += (int64_t)8 * s) cs_node(a, (int)i, s, e, lane);
        __syncthreads();
    }
}

// the 6x6 outputs from the supernode blocks: one thread per entry of a frame's three blocks; the padded frame of an odd F is never written
__global__ void __launch_bounds__(256) k_cv_sel_unpack(const double *S, const double *R, int F, double *fc, double *lc, double *l2) {
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= (int64_t)36 * F) return;
    const int f = (int)(t / 36), en = (int)(t % 36), r = en / 6, c = en % 6, k = f >> 1, o = 6 * (f & 1);
    const double *s = S + 144 * (size_t)k, *rr = R + 144 * (size_t)k;
    fc[t] = s[12 * (o + r) + o + c];
    if (f + 1 < F) lc[t] = o ? rr[12 * (6 + r) + c] : s[12 * r + 6 + c];
    if (f + 2 < F) l2[t] = rr[12 * (o + r) + o + c];
}

}  // namespace

size_t smooth_cv_selinv_doubles(int F) { return (size_t)smooth_cv_nodes(std::max(F, 1)) * 3 * 144 + (size_t)std::max(F, 1) * 3 * 36; }

int smooth_cv_selinv_launches(int F) { return F == 0 ? 0 : 2 + cv_own_levels(smooth_cv_nodes(F)); }

// after launch_smooth_cv_eval(.., true, ..) and launch_smooth_cv_solve(w, F, 0.0, st) on the same stream, on a zeroed area of
// smooth_cv_selinv_doubles(F) doubles: fc [F][36] = (H^-1)_ff, lc [F][36] with lc[f] = (H^-1)_{f,f+1} for f < F - 1, l2 [F][36] with
// l2[f] = (H^-1)_{f,f+2} for f < F - 2; a root pivot that is not positive beyond its rounding level raises w.flag.  Returns its launches.
int launch_smooth_cv_selinv(const SmoothCvWork &w, int F, double *area, double **fc, double **lc, double **l2, hipStream_t st) {
    if (F == 0) return 0;
    const int K = smooth_cv_nodes(F), n = cv_own_levels(K);
    CvSelArgs a;
    a.Dg = w.Dg; a.Dw = w.Dw; a.Uw = w.Uw; a.Dinv = w.Dinv; a.Ls = w.Ls; a.flag = w.flag; a.F = F; a.K = K;
    a.S = area; a.R[0] = area + 144 * (size_t)K; a.R[1] = area + 288 * (size_t)K;
    *fc = area + 432 * (size_t)K; *lc = *fc + 36 * (size_t)F; *l2 = *lc + 36 * (size_t)F;
    hipLaunchKernelGGL(k_cv_sel_tail, dim3(1), dim3(256), 0, st, a, 1 << n);   // the strides launch_smooth_cv_solve's tail ran
    for (int l = n - 1; l >= 0; l--) hipLaunchKernelGGL(k_cv_sel_level, dim3((cv_evens(K, 1 << l) + 3) / 4), dim3(256), 0, st, a, 1 << l, l);
    hipLaunchKernelGGL(k_cv_sel_unpack, dim3((unsigned)((36 * (int64_t)F + 255) / 256)), dim3(256), 0, st, a.S, a.R[0], F, *fc, *lc, *l2);
    return smooth_cv_selinv_launches(F);
}

}  // namespace aar
