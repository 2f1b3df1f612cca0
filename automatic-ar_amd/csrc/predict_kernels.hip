// Predicted marker corners with covariance, and the leverage of every detection (aar_problem_predict_corners,
// aar_problem_detection_leverage): the joint covariance of one (camera, marker, frame) triple pushed through the projection.
// See DESIGN.md section 36.
//
//   k_predict_gains    G_s = V_f^-1 W_s^T of every slot of every frame, columns of rows without an unknown zeroed (the gains of
//                      k_cov_frames, kept in memory: a frame's gains serve every query of that frame)
//   k_predict_corners  one wavefront per query.  Lanes 0-3 project one corner each and leave u (8) and G = du/dtheta (8 x 18) in LDS;
//                      lanes 0-35 own one entry (p, j) of Sigma_fc and of Sigma_fm, summed over the frame's slots in slot order;
//                      the 18 x 18 Sigma is gathered into LDS (entity blocks from the lower triangle of Sinv, the frame block from
//                      k_cov_frames' buffer, every pair (i, j), (j, i) from one value); T = G Sigma (144 entries over the lanes,
//                      18 terms each in index order); C = T G^T, its 36 entries r <= s on 36 lanes, each written to (r, s) and (s, r).
//                      Modes 3 and 4 keep C in LDS and run a tail behind it: A = I - C (3) or I + C (4), its
//                      Cholesky factor in LDS (lane (i, j) owns entry (i, j), columns in order, no pivoting), A w = r by lane 0, r^T w and
//                      w^T C w in index order, the smallest pivot, and for mode 3 F, Cook's distance and keep from the call's scalars.
// Rows and columns of Sinv without an unknown are read as ZERO (k_cov_stage made them identity rows).  fp64 throughout, no atomics,
// no cross-lane reduction: every sum has one owner and an order that does not depend on the launch.
#include "geom.hpp"
#include "kernels.h"

namespace aar {

__global__ void __launch_bounds__(64) k_predict_gains(const int32_t *__restrict__ fslot_start, const int32_t *__restrict__ fslot_ent,
                                                      const double *__restrict__ W, const double *__restrict__ Vinv,
                                                      const int32_t *__restrict__ rowmask, int F, double *__restrict__ gain) {
    const int f = blockIdx.x, lane = threadIdx.x;
    if (f >= F) return;
    const int s0 = fslot_start[f], ks = fslot_start[f + 1] - s0;
    for (int e = lane; e < ks * 36; e += 64) {
        const int s = e / 36, p = (e % 36) / 6, q = e % 6;   // G_s[p][q] = sum_r Vinv[p][r] W_s[q][r]
        const int a = fslot_ent[s0 + s];
        double v = 0.0;
        if (!rowmask[6 * a + q]) {
            const double *w = W + (size_t)(s0 + s) * 36 + q * 6, *vi = Vinv + (size_t)f * 36 + p * 6;
#pragma unroll
            for (int r = 0; r < 6; r++) v = fma(vi[r], w[r], v);
        }
        gain[(size_t)s0 * 36 + e] = v;
    }
}

namespace {

// Sinv(r, c) from the stored lower triangle; a row or column without an unknown reads as zero
__device__ __forceinline__ double sinv_at(const PredictArgs &a, int r, int c) {
    if (a.rowmask[r] || a.rowmask[c]) return 0.0;
    return r >= c ? a.Sinv[(size_t)r * a.n_pad + c] : a.Sinv[(size_t)c * a.n_pad + r];
}

}  // namespace

// MODE 0: explicit queries, uv | cov | status.  MODE 1: explicit queries, uv | status only (no covariance chain behind it).
// MODE 2: the problem's own detections (ordering A = reference order), trace and diagonal of C | status.
// MODE 3: the problem's own detections, leave-one-out: r = observed - u, A = I - C, w = A^-1 r | q | F | cook | leverage | margin | status | keep.
// MODE 4: explicit queries with observed corners, the gate: e = observed - u, A = I + C, e | e^T A^-1 e | margin | status.
template <int MODE>
__global__ void __launch_bounds__(64) k_predict_corners(const PredictArgs a) {
    __shared__ double sG[8][18], sSig[18][19], sT[8][19], sUV[8], sDiag[8];
    __shared__ double sC[8][9], sA[8][9], sL[8], sR[8];   // (modes 3, 4 only)
    __shared__ int sBehind[4];
    const int64_t q = blockIdx.x;
    const int lane = threadIdx.x;
    if (q >= a.n) return;
    int c, em, f;
    if (MODE == 2 || MODE == 3) {
        const ObsIdx o = a.obs[q];
        c = o.cam; em = o.marker; f = o.frame;
    } else {
        c = a.q_cam[q]; em = a.C + a.q_marker[q]; f = a.q_frame[q];
    }
    if (lane < 4) {
        Ent ec, emk, ef;
        load_ent(a.ent, c, ec);
        load_ent(a.ent, em, emk);
        load_ent(a.ent, a.A + f, ef);
        const double *K = a.K + (size_t)a.kstride * c;
        CornerGeom g;
        project_corner(ec, emk, ef, K, a.h, lane, g);
        sUV[2 * lane] = g.u;
        sUV[2 * lane + 1] = g.v;
        sBehind[lane] = !(g.pc[2] > 0.0);
        if (MODE != 1) {
            double Gc[2][6], Gm[2][6], Gf[2][6];
            corner_jacobian<true, true, true>(ec, emk, ef, K, g, Gc, Gm, Gf);
#pragma unroll
            for (int r = 0; r < 2; r++)
#pragma unroll
                for (int j = 0; j < 6; j++) {
                    sG[2 * lane + r][j] = Gc[r][j];
                    sG[2 * lane + r][6 + j] = Gm[r][j];
                    sG[2 * lane + r][12 + j] = Gf[r][j];
                }
        }
    }
    __syncthreads();
    const double nan = __builtin_nan("");
    const int s0 = a.fslot_start[f], ks = a.fslot_start[f + 1] - s0;
    const int mc = a.rowmask[6 * c], mm = a.rowmask[6 * em];
    const bool behind = sBehind[0] || sBehind[1] || sBehind[2] || sBehind[3];
    const bool undefined = mc == PREDICT_UNSEEN || mm == PREDICT_UNSEEN || (a.frames_opt && ks == 0);
    if (lane == 0) a.status[q] = (uint8_t)((behind ? 1 : 0) | (undefined ? 2 : 0));
    if (MODE < 2 && lane < 8) a.uv[(size_t)q * 8 + lane] = behind ? nan : sUV[lane];
    if (MODE == 1) return;
    if (behind || undefined) {   // (the same for every lane: nobody waits at a barrier below)
        if (MODE == 0) a.cov[(size_t)q * 64 + lane] = nan;
        if (MODE == 2) {
            if (lane == 0) a.lev[q] = nan;
            if (a.row_lev && lane < 8) a.row_lev[(size_t)q * 8 + lane] = nan;
        }
        if (MODE >= 3) {
            // (the gate's innovation needs no covariance: it is NaN only where the corners themselves are)
            if (lane < 8) a.loo_w[(size_t)q * 8 + lane] = (MODE == 3 || behind) ? nan : (double)a.obs_uv[(size_t)q * 8 + lane] - sUV[lane];
            if (lane == 0) {
                a.loo_q[q] = nan;
                a.loo_margin[q] = nan;
                if (MODE == 3) { a.lev[q] = nan; a.loo_F[q] = nan; a.loo_cook[q] = nan; a.loo_keep[q] = 1; }
            }
        }
        return;
    }
    // Sigma_fc and Sigma_fm: lane (p, j) sums G_s[p][k] Sinv[6 ent(s) + k][6 e + j] over the frame's slots in slot order
    if (lane < 36) {
        const int p = lane / 6, j = lane % 6;
        double ac = 0.0, am = 0.0;
        if (a.frames_opt) {
            // (a masked ROW needs no test here: k_predict_gains zeroed that column of G, and the identity row S^-1 holds there is finite;
            // a masked COLUMN is zeroed behind the loop)
            const int cc = 6 * c + j, cm = 6 * em + j;
            const double *__restrict__ Sinv = a.Sinv;
            const size_t np = (size_t)a.n_pad;
#pragma unroll 4
            for (int s = 0; s < ks; s++) {
                const int r0 = 6 * a.fslot_ent[s0 + s];
                const double *__restrict__ g = a.gain + (size_t)(s0 + s) * 36 + p * 6;
#pragma unroll
                for (int k = 0; k < 6; k++) {
                    const int r = r0 + k;
                    const double gk = g[k];
                    ac = fma(gk, r >= cc ? Sinv[r * np + cc] : Sinv[cc * np + r], ac);
                    am = fma(gk, r >= cm ? Sinv[r * np + cm] : Sinv[cm * np + r], am);
                }
            }
            if (mc) ac = 0.0;
            if (mm) am = 0.0;
        }
        sSig[12 + p][j] = -ac; sSig[j][12 + p] = -ac;
        sSig[12 + p][6 + j] = -am; sSig[6 + j][12 + p] = -am;
    }
    // the entity blocks: the 78 entries i >= j of the 12 x 12 corner
    for (int t = lane; t < 78; t += 64) {
        int i = 0, j = t;
        while (j > i) { j -= i + 1; i++; }
        const int gi = i < 6 ? 6 * c + i : 6 * em + (i - 6), gj = j < 6 ? 6 * c + j : 6 * em + (j - 6);
        const double v = sinv_at(a, gi, gj);
        sSig[i][j] = v; sSig[j][i] = v;
    }
    // the frame block: the 21 entries p >= r of k_cov_frames' block (zero where the frames are constants)
    if (lane < 21) {
        int p = 0, r = lane;
        while (r > p) { r -= p + 1; p++; }
        const double v = a.frames_opt ? a.frame_cov[(size_t)f * 36 + p * 6 + r] : 0.0;
        sSig[12 + p][12 + r] = v; sSig[12 + r][12 + p] = v;
    }
    __syncthreads();
    for (int e = lane; e < 144; e += 64) {   // T = G Sigma
        const int r = e / 18, j = e % 18;
        double v = 0.0;
#pragma unroll
        for (int i = 0; i < 18; i++) v = fma(sG[r][i], sSig[i][j], v);
        sT[r][j] = v;
    }
    __syncthreads();
    if (lane < 36) {   // C = T G^T, entries r <= s
        int r = 0, t = lane;
        while (t >= 8 - r) { t -= 8 - r; r++; }
        const int s = r + t;
        double v = 0.0;
#pragma unroll
        for (int j = 0; j < 18; j++) v = fma(sT[r][j], sG[s][j], v);
        if (MODE == 0) {
            a.cov[(size_t)q * 64 + r * 8 + s] = v;
            a.cov[(size_t)q * 64 + s * 8 + r] = v;
        } else if (r == s) {
            sDiag[r] = v;
        }
        if (MODE >= 3) { sC[r][s] = v; sC[s][r] = v; }
    }
    if (MODE == 2) {
        __syncthreads();
        if (a.row_lev && lane < 8) a.row_lev[(size_t)q * 8 + lane] = sDiag[lane];
        if (lane == 0) a.lev[q] = ((sDiag[0] + sDiag[1]) + (sDiag[2] + sDiag[3])) + ((sDiag[4] + sDiag[5]) + (sDiag[6] + sDiag[7]));
    }
    if (MODE >= 3) {
        __syncthreads();
        if (MODE == 3 && lane == 0) a.lev[q] = ((sDiag[0] + sDiag[1]) + (sDiag[2] + sDiag[3])) + ((sDiag[4] + sDiag[5]) + (sDiag[6] + sDiag[7]));
        // A and r: lane (i, j) owns A[i][j] from here to the end of the factorisation
        const int i = lane >> 3, j = lane & 7;
        sA[i][j] = MODE == 3 ? (i == j ? 1.0 - sC[i][j] : -sC[i][j]) : (i == j ? 1.0 + sC[i][j] : sC[i][j]);
        if (lane < 8) sR[lane] = (double)a.obs_uv[(size_t)q * 8 + lane] - sUV[lane];
        // A = L L^T, right-looking, column by column: the pivot stays where it is (its root goes to sL), column k is scaled by its owners,
        // the trailing lower triangle is updated by its owners.  Every lane reads the same pivot: the loop ends for all of them together
        double margin = __builtin_inf();
        bool bad = false;
        for (int k = 0; k < 8; k++) {
            __syncthreads();
            const double d = sA[k][k];
            if (!(d >= margin)) margin = d;
            if (!(d > PREDICT_LOO_MIN_PIVOT) || !(d < __builtin_inf())) { bad = true; break; }
            const double l = sqrt(d);
            if (j == k && i > k) sA[i][k] = sA[i][k] / l;
            if (lane == 9 * k) sL[k] = l;
            __syncthreads();
            if (j > k && i >= j) sA[i][j] = fma(-sA[i][k], sA[j][k], sA[i][j]);
        }
        __syncthreads();
        if (lane == 0) {
            double w[8], qv = nan, kv = nan;
            if (!bad) {
                double y[8];
#pragma unroll
                for (int r = 0; r < 8; r++) {   // L y = r
                    double v = sR[r];
#pragma unroll
                    for (int c2 = 0; c2 < r; c2++) v = fma(-sA[r][c2], y[c2], v);
                    y[r] = v / sL[r];
                }
#pragma unroll
                for (int r = 7; r >= 0; r--) {   // L^T w = y
                    double v = y[r];
#pragma unroll
                    for (int c2 = 7; c2 > r; c2--) v = fma(-sA[c2][r], w[c2], v);
                    w[r] = v / sL[r];
                }
                qv = 0.0;
                kv = 0.0;
#pragma unroll
                for (int r = 0; r < 8; r++) qv = fma(sR[r], w[r], qv);
#pragma unroll
                for (int r = 0; r < 8; r++) {
                    double t = 0.0;
#pragma unroll
                    for (int c2 = 0; c2 < 8; c2++) t = fma(sC[r][c2], w[c2], t);
                    kv = fma(w[r], t, kv);
                }
            } else {
#pragma unroll
                for (int r = 0; r < 8; r++) w[r] = nan;
                a.status[q] = (uint8_t)PREDICT_UNDETERMINED;   // (bits 0 and 1 are clear on this path)
            }
#pragma unroll
            for (int r = 0; r < 8; r++) a.loo_w[(size_t)q * 8 + r] = MODE == 3 ? w[r] : sR[r];
            a.loo_q[q] = qv;
            a.loo_margin[q] = margin;
            if (MODE == 3) {
                double Fv = nan;
                if (!bad && a.dof > 8) {
                    const double den = (a.sum_sq - qv) / (double)(a.dof - 8);
                    Fv = den <= 0.0 ? __builtin_inf() : (qv / 8.0) / den;
                }
                a.loo_k[q] = kv;
                a.loo_F[q] = Fv;
                a.loo_cook[q] = kv / a.cook_den;
                a.loo_keep[q] = (a.f_max > 0.0 && !bad && Fv > a.f_max) ? 0 : 1;
            }
        }
    }
}

void launch_predict_gains(const DeviceProblem &P, int which, const int32_t *rowmask, double *gain, hipStream_t st) {
    if (P.F == 0) return;
    hipLaunchKernelGGL(k_predict_gains, dim3((unsigned)P.F), dim3(64), 0, st, P.fslot_start, P.fslot_ent, P.blk[which].W, P.blk[which].Vinv, rowmask,
                       P.F, gain);
}

void launch_predict_corners(const PredictArgs &a, int mode, hipStream_t st) {
    if (a.n <= 0) return;
    const dim3 grid((unsigned)a.n), block(64);
    if (mode == 0) hipLaunchKernelGGL(k_predict_corners<0>, grid, block, 0, st, a);
    else if (mode == 1) hipLaunchKernelGGL(k_predict_corners<1>, grid, block, 0, st, a);
    else if (mode == 2) hipLaunchKernelGGL(k_predict_corners<2>, grid, block, 0, st, a);
    else if (mode == 3) hipLaunchKernelGGL(k_predict_corners<3>, grid, block, 0, st, a);
    else hipLaunchKernelGGL(k_predict_corners<4>, grid, block, 0, st, a);
}

}  // namespace aar
