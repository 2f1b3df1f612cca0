// Smoothed tracks: the covariance between ANY two frames and the relative motion with its 6x6 covariance.
// H is block tridiagonal in frames under the random walk and block tridiagonal in supernodes under constant velocity, so the posterior is a
// Gauss-Markov chain:
//   Sigma_ab = Sigma_ak Sigma_kk^-1 Sigma_kb  for a < k < b,  hence  Sigma_ab = Sigma_{a,a+1} C_{a+1} ... C_{b-1},  C_k = Sigma_kk^-1 Sigma_{k,k+1}
// on frames (6x6) or supernodes (12x12).  Everything it needs is what the selected inverses leave on the device:
//   random walk        S[f] = (H^-1)_ff, R[f] = (H^-1)_{f,f+1}              (launch_smooth_selinv)
//   constant velocity  S[K], R[K] the same on supernodes K = frames (2K, 2K + 1), 12x12, and the 6x6 blocks fc, lc, l2, l3 by lag
//                      (launch_smooth_cv_selinv, launch_smooth_cv_lag3)
//
//   k_smooth_gain         one thread per inner frame k = 1 .. F-2: C_k = S_k^-1 R_k by spd6_inverse
//   k_smooth_relative     one thread per query: X = R_lo, X <- X C_k for k = lo+1 .. hi-1 (lo = min(a, b), hi = max(a, b)); lags 0 and 1 copy
//   k_smooth_cv_gain      one wavefront per inner supernode K = 1 .. Kn-2 in the row layout of cv_rows.hpp: C_K = S_K^-1 R_K
//   k_smooth_cv_relative  one wavefront per query: lane i holds row i of X = R_Ka C_{Ka+1} ... C_{Kb-1}; the answer is its 6x6 sub-block
//                         (lo mod 2, hi mod 2).  Lags 0 .. 3 copy fc, lc, l2, l3 (every pair of the same or of neighbouring supernodes is one)
// The padded frame of an odd F sits in the LAST supernode, which no chain inverts (the chain inverts Ka+1 .. Kb-1 <= Kn-2) and whose padded
// columns no query reads.
//
// Then, for both models alike (rel_answers), with z_a, z_b the two poses and phi, e_t, M_a, M_b of pair_terms<true> WITHOUT an expected motion:
//   rel     = [phi ; e_t] = [log(R_a^T R_b) ; t_b - t_a]
//   rel_cov = J_a S_aa J_a^T + J_b S_bb J_b^T + J_a S_ab J_b^T + J_b S_ab^T J_a^T,   J_a = [M_a 0; 0 -I],  J_b = [M_b 0; 0 I]
// in 3x3 sub-blocks, the four summands added in this order, the lower triangle computed and mirrored.  a = b: zeros.
// fp64, no atomics, no LDS, every sum in ascending order, one owner per store: a query's bits depend on (a, b) and the track alone.
#include "cv_rows.hpp"
#include "geom.hpp"
#include "kernels.h"
#include "pair_terms.hpp"
#include "so3.hpp"

namespace aar {

namespace {

struct RelArgs {
    const double *z;                  // [F][6] frame poses
    const double *S, *R;              // random walk: [F][36] each; constant velocity: [Kn][144] each
    double *C;                        // the gains, in the same shape
    const double *fc, *lc, *l2, *l3;  // constant velocity: the 6x6 blocks by lag
    const int32_t *fa, *fb;           // [Q] the pairs
    double *cross, *rel, *rcov;       // [Q][36], [Q][6], [Q][36]
    int32_t *flag;                    // raised by a non-positive pivot of a gain
    int F, K;
    int64_t Q;
};

// sum_kl L(i,k) B(k,l) R(j,l) with B the 3x3 sub-block (br, bc) of the 6x6 block s, or (TR) the transpose of its sub-block (bc, br)
template <bool TR>
__device__ __forceinline__ double lsr(const double *L, int i, const double *s, int br, int bc, const double *R, int j) {
    double t = 0.0;
#pragma unroll
    for (int k = 0; k < 3; k++) {
        double u = 0.0;
#pragma unroll
        for (int l = 0; l < 3; l++) u = fma(TR ? s[6 * (3 * bc + l) + 3 * br + k] : s[6 * (3 * br + k) + 3 * bc + l], R[3 * j + l], u);
        t = fma(L[3 * i + k], u, t);
    }
    return t;
}

// rel and rel_cov of the pair (fa, fb), fa != fb, from X = Sigma_ab (rows: frame fa) and the diagonal blocks saa, sbb; st: this lane stores
__device__ __forceinline__ void rel_answers(const double *z, int fa, int fb, const double *saa, const double *sbb, const double *X, bool st,
                                            double *rel, double *rcov) {
    double za[6], zb[6], ra[ENT_STRIDE], rb[ENT_STRIDE], phi[3], et[3];
    double JA[2][9], JB[2][9];
    ld6(z + 6 * (size_t)fa, za);
    ld6(z + 6 * (size_t)fb, zb);
    make_ent_row(za, ra);
    make_ent_row(zb, rb);
    pair_terms<true>(ra, rb, nullptr, phi, et, JA[0], JB[0]);
#pragma unroll
    for (int i = 0; i < 9; i++) {
        JA[1][i] = i % 4 == 0 ? -1.0 : 0.0;
        JB[1][i] = i % 4 == 0 ? 1.0 : 0.0;
    }
    if (st) {
#pragma unroll
        for (int i = 0; i < 3; i++) { rel[i] = phi[i]; rel[3 + i] = et[i]; }
    }
#pragma unroll
    for (int br = 0; br < 2; br++)
#pragma unroll
        for (int bc = 0; bc <= br; bc++)
#pragma unroll
            for (int i = 0; i < 3; i++)
#pragma unroll
                for (int j = 0; j < 3; j++) {
                    if (br == bc && j > i) continue;
                    double v = lsr<false>(JA[br], i, saa, br, bc, JA[bc], j);
                    v += lsr<false>(JB[br], i, sbb, br, bc, JB[bc], j);
                    v += lsr<false>(JA[br], i, X, br, bc, JB[bc], j);
                    v += lsr<true>(JB[br], i, X, br, bc, JA[bc], j);
                    if (st) {
                        rcov[6 * (3 * br + i) + 3 * bc + j] = v;
                        rcov[6 * (3 * bc + j) + 3 * br + i] = v;
                    }
                }
}

// a = b: the frame's own block, no motion and no uncertainty of it
__device__ __forceinline__ void rel_same(const double *saa, double *cross, double *rel, double *rcov) {
#pragma unroll
    for (int i = 0; i < 36; i++) { cross[i] = saa[i]; rcov[i] = 0.0; }
#pragma unroll
    for (int i = 0; i < 6; i++) rel[i] = 0.0;
}

__global__ void __launch_bounds__(64) k_smooth_gain(const RelArgs a) {
    const int k = blockIdx.x * 64 + threadIdx.x + 1;
    if (k + 1 >= a.F) return;
    double m[6][6], I[36];
    const double *s = a.S + 36 * (size_t)k, *r = a.R + 36 * (size_t)k;
#pragma unroll
    for (int i = 0; i < 6; i++)
#pragma unroll
        for (int j = 0; j < 6; j++) m[i][j] = s[6 * i + j];
    if (!spd6_inverse(m, I)) a.flag[0] = 1;
    double *c = a.C + 36 * (size_t)k;
#pragma unroll
    for (int j = 0; j < 6; j++) {
        double x[6];
#pragma unroll
        for (int p = 0; p < 6; p++) x[p] = r[6 * p + j];
#pragma unroll
        for (int i = 0; i < 6; i++) {
            double t = 0.0;
#pragma unroll
            for (int p = 0; p < 6; p++) t = fma(I[6 * i + p], x[p], t);
            c[6 * i + j] = t;
        }
    }
}

__global__ void __launch_bounds__(64) k_smooth_relative(const RelArgs a) {
    const int64_t q = (int64_t)blockIdx.x * 64 + threadIdx.x;
    if (q >= a.Q) return;
    const int fa = a.fa[q], fb = a.fb[q], lo = fa < fb ? fa : fb, hi = fa < fb ? fb : fa;
    double *cross = a.cross + 36 * (size_t)q, *rel = a.rel + 6 * (size_t)q, *rcov = a.rcov + 36 * (size_t)q;
    if (lo == hi) { rel_same(a.S + 36 * (size_t)fa, cross, rel, rcov); return; }
    double X[36];
#pragma unroll
    for (int i = 0; i < 36; i++) X[i] = a.R[36 * (size_t)lo + i];
#pragma unroll 1
    for (int k = lo + 1; k < hi; k++) {
        const double *c = a.C + 36 * (size_t)k;
#pragma unroll
        for (int r = 0; r < 6; r++) {
            double x[6];
#pragma unroll
            for (int p = 0; p < 6; p++) x[p] = X[6 * r + p];
#pragma unroll
            for (int j = 0; j < 6; j++) {
                double t = 0.0;
#pragma unroll
                for (int p = 0; p < 6; p++) t = fma(x[p], c[6 * p + j], t);
                X[6 * r + j] = t;
            }
        }
    }
    if (fa > fb) {
#pragma unroll
        for (int i = 0; i < 5; i++)
#pragma unroll
            for (int j = i + 1; j < 6; j++) {
                const double t = X[6 * i + j];
                X[6 * i + j] = X[6 * j + i];
                X[6 * j + i] = t;
            }
    }
#pragma unroll
    for (int i = 0; i < 36; i++) cross[i] = X[i];
    rel_answers(a.z, fa, fb, a.S + 36 * (size_t)fa, a.S + 36 * (size_t)fb, X, true, rel, rcov);
}

__global__ void __launch_bounds__(256) k_smooth_cv_gain(const RelArgs a) {
    const int lane = threadIdx.x & 63, k = blockIdx.x * 4 + wave_of_block() + 1;
    if (k + 1 >= a.K) return;
    const int ri = lane < 12 ? lane : 11;
    double I[12], B[12], Cr[12];
    ld_row(a.S + 144 * (size_t)k, ri, I);
    const bool ok = row_inverse(ri, I);
    ld_row(a.R + 144 * (size_t)k, ri, B);
    row_mm<false>(I, B, 1.0, Cr);
    st_row(a.C + 144 * (size_t)k, lane, Cr);
    if (!ok && lane == 0) a.flag[0] = 1;
}

__global__ void __launch_bounds__(256) k_smooth_cv_relative(const RelArgs a) {
    const int lane = threadIdx.x & 63;
    const int64_t q = (int64_t)blockIdx.x * 4 + wave_of_block();   // wave-uniform, as everything below that does not name the lane
    if (q >= a.Q) return;
    const int fa = __builtin_amdgcn_readfirstlane(a.fa[q]), fb = __builtin_amdgcn_readfirstlane(a.fb[q]);
    const int lo = fa < fb ? fa : fb, hi = fa < fb ? fb : fa, lag = hi - lo;
    double *cross = a.cross + 36 * (size_t)q, *rel = a.rel + 6 * (size_t)q, *rcov = a.rcov + 36 * (size_t)q;
    if (lag == 0) {
        if (lane == 0) rel_same(a.fc + 36 * (size_t)fa, cross, rel, rcov);
        return;
    }
    double X[36];   // Sigma_{lo,hi}, the same in every lane
    if (lag <= 3) {
        const double *blk = (lag == 1 ? a.lc : lag == 2 ? a.l2 : a.l3) + 36 * (size_t)lo;
#pragma unroll
        for (int i = 0; i < 36; i++) X[i] = blk[i];
    } else {
        const int ri = lane < 12 ? lane : 11, ka = lo >> 1, kb = hi >> 1;
        double P[12], Cr[12], T[12];
        ld_row(a.R + 144 * (size_t)ka, ri, P);
#pragma unroll 1
        for (int k = ka + 1; k < kb; k++) {
            ld_row(a.C + 144 * (size_t)k, ri, Cr);
            row_mm<false>(P, Cr, 1.0, T);
#pragma unroll
            for (int j = 0; j < 12; j++) P[j] = T[j];
        }
        // the sub-block (lo mod 2, hi mod 2): rows from the lanes that hold them, the column half chosen by every lane alike
        const int ro = 6 * (lo & 1);
        const bool right = (hi & 1) != 0;
#pragma unroll
        for (int r = 0; r < 6; r++)
#pragma unroll
            for (int c = 0; c < 6; c++) X[6 * r + c] = bc(right ? P[6 + c] : P[c], ro + r);
    }
    if (fa > fb) {
#pragma unroll
        for (int i = 0; i < 5; i++)
#pragma unroll
            for (int j = i + 1; j < 6; j++) {
                const double t = X[6 * i + j];
                X[6 * i + j] = X[6 * j + i];
                X[6 * j + i] = t;
            }
    }
    if (lane == 0) {
#pragma unroll
        for (int i = 0; i < 36; i++) cross[i] = X[i];
    }
    rel_answers(a.z, fa, fb, a.fc + 36 * (size_t)fa, a.fc + 36 * (size_t)fb, X, lane == 0, rel, rcov);
}

}  // namespace

// Random walk, after launch_smooth_selinv(.., S, R, st) on the same stream (F > 0, Q > 0): the answers of the pairs (fa[q], fb[q]) into cross
// [Q][36], rel [Q][6], rcov [Q][36].  C [F][36] takes the gains and is written only with chained = true (some pair has a lag above 1); a
// non-positive pivot of a gain's S_k sets flag[0] = 1 (the caller zeroes it).  All pointers on the device.  Returns its launches.
int launch_smooth_relative(int F, const double *z, const double *S, const double *R, double *C, bool chained, int64_t Q, const int32_t *fa,
                           const int32_t *fb, double *cross, double *rel, double *rcov, int32_t *flag, hipStream_t st) {
    RelArgs a;
    a.z = z; a.S = S; a.R = R; a.C = C; a.fc = a.lc = a.l2 = a.l3 = nullptr; a.fa = fa; a.fb = fb; a.cross = cross; a.rel = rel; a.rcov = rcov;
    a.flag = flag; a.F = F; a.K = 0; a.Q = Q;
    int launches = 0;
    if (chained && F > 2) {
        hipLaunchKernelGGL(k_smooth_gain, dim3((F - 2 + 63) / 64), dim3(64), 0, st, a);
        launches++;
    }
    hipLaunchKernelGGL(k_smooth_relative, dim3((unsigned)((Q + 63) / 64)), dim3(64), 0, st, a);
    return launches + 1;
}

// Constant velocity, after launch_smooth_cv_selinv on area and launch_smooth_cv_lag3 on the same stream (F > 0, Q > 0): the same answers.
// area holds S and R of the supernodes at its start; fc, lc, l2, l3 the 6x6 blocks by lag; C [Kn][144] takes the gains, written only with
// chained = true (some pair has a lag above 3).
int launch_smooth_cv_relative(int F, const double *z, const double *area, const double *fc, const double *lc, const double *l2, const double *l3,
                              double *C, bool chained, int64_t Q, const int32_t *fa, const int32_t *fb, double *cross, double *rel, double *rcov,
                              int32_t *flag, hipStream_t st) {
    RelArgs a;
    a.F = F; a.K = smooth_cv_nodes(F); a.Q = Q;
    a.z = z; a.S = area; a.R = area + 144 * (size_t)a.K; a.C = C; a.fc = fc; a.lc = lc; a.l2 = l2; a.l3 = l3; a.fa = fa; a.fb = fb;
    a.cross = cross; a.rel = rel; a.rcov = rcov; a.flag = flag;
    int launches = 0;
    if (chained && a.K > 2) {
        hipLaunchKernelGGL(k_smooth_cv_gain, dim3((a.K - 2 + 3) / 4), dim3(256), 0, st, a);
        launches++;
    }
    hipLaunchKernelGGL(k_smooth_cv_relative, dim3((unsigned)((Q + 3) / 4)), dim3(256), 0, st, a);
    return launches + 1;
}

}  // namespace aar
