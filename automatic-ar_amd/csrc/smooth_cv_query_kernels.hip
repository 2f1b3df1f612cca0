// The constant-velocity smoothed track at any time: pose and 6x6 covariance block at query times that are not frame
// times, defined as what ONE Gauss-Newton step of the constant-velocity smoother (section 31) reports for a frame m WITHOUT detections inserted
// at the query's time, linearised at the track with m at a start pose.  Inputs are what aar_track_smooth_covariance2 leaves on the device: the
// frame poses z, fc[f] = (H^-1)_ff, lc[f] = (H^-1)_{f,f+1}, l2[f] = (H^-1)_{f,f+2} (launch_smooth_cv_selinv) and, new here, l3[f] = (H^-1)_{f,f+3}.
//
// k_cv_lag3: the lag-three blocks from the supernode blocks S, R of the selected inverse (supernode k = frames 2k, 2k + 1), one wavefront per
// supernode in the row layout of cv_rows.hpp:
//   even f = 2k       l3[f] = R[k][0:6, 6:12]                                       (the block k_cv_sel_unpack drops)
//   odd  f = 2k - 1   l3[f] = (R[k-1] S[k]^-1 R[k])[6:12, 0:6]                      (Sigma_{k-1,k+1} = Sigma_{k-1,k} Sigma_kk^-1 Sigma_{k,k+1}: the
//                                                                                    Gauss-Markov property of a block-tridiagonal H)
//
// k_smooth_cv_query: ONE WAVEFRONT PER QUERY, four per workgroup, fp64.  The frames around the query sit at FIXED local slots
//   slot 0 .. 3 = frames fb .. fb + 3 where they exist (inside the gap (a, a + 1): fb = a - 1; after the end: fb = F - 2; before the start:
//   fb = -2), slot 4 = m
// so that every changed term has compile-time slots and a lane's row never needs a computed register index:
//   removed   term (0, 1, 2) if a >= 1, term (1, 2, 3) if a + 1 <= F - 2, pair (1, 2) if a = 0            before the start: pair (2, 3)
//   added     term (0, 1, 4) [also after the end], term (1, 4, 2), term (4, 2, 3) [also before the start],
//             pair (1, 4) if a = 0 [also after the end of a one-frame track]                              before the start: pair (4, 2)
// Lane i holds row i of the local matrix (row 6 s + l = entry l of slot s); a slot without a frame is an identity row and column.
//   1. P = Sigma_NN gathered from fc, lc, l2, l3 by frame index (24x24), inverted in place by Gauss-Jordan: the neighbours' marginal information
//   2. rows widened to 30: K = P^-1 - F_old, then + F_new; every lane adds its own row of each term's J^T L J and its entry of d = g' - g
//      (the terms themselves -- cv_term<true>, pair_terms<true> -- are computed by every lane alike, as k_smooth_cv_eval does)
//   3. rows 0 .. 23 eliminated from the rows below (no pivoting, the right-hand side carried): rows 24 .. 29 hold C - B^T A^-1 B and
//      d_m - B^T A^-1 d_N
//   4. that 6x6 block inverted by Gauss-Jordan among lanes 24 .. 29, its upper triangle replaced by the lower one: cov; delta_m = cov times the
//      reduced right-hand side; pose = start pose + delta_m, as the smoother's trial point applies a step
// Operand rows travel by constant-lane v_readlane, every sum runs in ascending order, no LDS, no atomics, nothing shared between queries: a
// query's bits depend on its time and the track alone.  A non-positive pivot anywhere raises the flag with a plain store.
#include "cv_rows.hpp"
#include "cv_term.hpp"
#include "geom.hpp"
#include "kernels.h"
#include "pair_terms.hpp"
#include "so3.hpp"

namespace aar {

namespace {

struct CvLag3Args {
    const double *S, *R;   // [K][144] each: the selected inverse's supernode blocks after stride 1
    double *l3;            // [F - 3][36]
    int32_t *flag;
    int F, K;
};

__global__ void __launch_bounds__(256) k_cv_lag3(const CvLag3Args a) {
    const int lane = threadIdx.x & 63, k = blockIdx.x * 4 + wave_of_block();
    if (k >= a.K) return;
    const int ri = lane < 12 ? lane : 11;
    if (2 * k + 3 < a.F && lane < 36) a.l3[36 * (size_t)(2 * k) + lane] = a.R[144 * (size_t)k + 12 * (lane / 6) + 6 + lane % 6];
    if (k >= 1 && 2 * k + 2 < a.F) {
        double I[12], A[12], T[12], B[12], U[12];
        ld_row(a.S + 144 * (size_t)k, ri, I);
        const bool ok = row_inverse(ri, I);
        ld_row(a.R + 144 * (size_t)(k - 1), ri, A);
        row_mm<false>(A, I, 1.0, T);
        ld_row(a.R + 144 * (size_t)k, ri, B);
        row_mm<false>(T, B, 1.0, U);
        if (lane >= 6 && lane < 12) {
            double *o = a.l3 + 36 * (size_t)(2 * k - 1) + 6 * (lane - 6);
#pragma unroll
            for (int j = 0; j < 6; j++) o[j] = U[j];
        }
        if (!ok && lane == 0) a.flag[0] = 1;
    }
}

struct CvQueryArgs {
    const double *z;                  // [F][6] frame poses
    const double *ft;                 // [F] frame times, ascending
    const double *fc, *lc, *l2, *l3;  // [F][36] each ([F - 3][36] the last): the blocks of H^-1 by lag
    const double *qt;                 // [Q] query times
    double *pose, *cov;               // [Q][6], [Q][36]
    double *start, *step;             // [Q][6] each or NULL: the start pose and delta_m on their own
    int32_t *seg;                     // [Q]
    int32_t *flag;                    // raised by a non-positive pivot
    double sr2, st2, sr02, st02;      // the sigmas, squared
    int F;
    int64_t Q;
};

__device__ __forceinline__ double sel3(int i, double x, double y, double z) { return i == 0 ? x : i == 1 ? y : z; }

// cv_rows.hpp's Gauss-Jordan inverse on N rows: lane i < N holds row i
template <int N>
__device__ __forceinline__ bool rown_inverse(int ri, double *a) {
    bool ok = true;
#pragma unroll
    for (int k = 0; k < N; k++) {
        double pr[N];
#pragma unroll
        for (int j = 0; j < N; j++) pr[j] = bc(a[j], k);
        const double p = pr[k];
        ok = ok && p > 0.0;
        const double ip = 1.0 / p, f = a[k];
        const bool own = ri == k;
#pragma unroll
        for (int j = 0; j < N; j++) {
            const double s = pr[j] * ip;
            if (j != k) a[j] = own ? s : fma(-f, s, a[j]);
        }
        a[k] = own ? ip : -f * ip;
    }
    return ok;
}

// rows 0 .. NE-1 of an N x N positive definite matrix eliminated from the rows below them, the right-hand side d carried: rows NE .. N-1 end
// with the Schur complement in their columns NE .. N-1 and the reduced right-hand side
template <int N, int NE>
__device__ __forceinline__ bool rown_eliminate(int ri, double *a, double &d) {
    bool ok = true;
#pragma unroll
    for (int k = 0; k < NE; k++) {
        const double p = bc(a[k], k);
        ok = ok && p > 0.0;
        const double f = a[k] * (1.0 / p);
        const bool below = ri > k;
#pragma unroll
        for (int j = k + 1; j < N; j++) {
            const double pj = bc(a[j], k);
            if (below) a[j] = fma(-f, pj, a[j]);
        }
        const double pd = bc(d, k);
        if (below) d = fma(-f, pd, d);
    }
    return ok;
}

// this lane's row gains sg * (column block S of one term's J^T L J): col = column l of the lane's own Jacobian block (l < 3), cx its translation
// coefficient; (My, cy) the Jacobian block of the frame at slot S
template <int S>
__device__ __forceinline__ void q_block(double *a, bool rot, int li, double sg, double lr, double lt, const double *col, double cx, const double *My,
                                        double cy) {
    if (rot) {
#pragma unroll
        for (int j = 0; j < 3; j++) a[6 * S + j] += sg * (lr * (col[0] * My[j] + col[1] * My[3 + j] + col[2] * My[6 + j]));
    } else {
        const double v = sg * (lt * cx * cy);
#pragma unroll
        for (int j = 3; j < 6; j++)
            if (li == j) a[6 * S + j] += v;
    }
}

// one changed term into this lane's row and its entry of d = g' - g: the term's frames sit at the slots S0, S1, S2 (S2 < 0: a pair), its Jacobian
// blocks are [M 0; 0 c I]; sg = +1 an added term, -1 a removed one
template <int S0, int S1, int S2>
__device__ __forceinline__ void q_acc(double *a, double &d, int slot, int li, double sg, double lr, double lt, const double *phi, const double *et,
                                      const double *M0, double c0, const double *M1, double c1, const double *M2, double c2) {
    const bool i0 = slot == S0, i1 = slot == S1, i2 = S2 >= 0 && slot == S2;
    if (!(i0 || i1 || i2)) return;
    double col[3];
#pragma unroll
    for (int k = 0; k < 3; k++) {
        const double m0 = sel3(li, M0[3 * k], M0[3 * k + 1], M0[3 * k + 2]), m1 = sel3(li, M1[3 * k], M1[3 * k + 1], M1[3 * k + 2]),
                     m2 = sel3(li, M2[3 * k], M2[3 * k + 1], M2[3 * k + 2]);
        col[k] = i0 ? m0 : i1 ? m1 : m2;
    }
    const double cx = i0 ? c0 : i1 ? c1 : c2;
    const bool rot = li < 3;
    // rhs = -J^T L e: an added term enters g', a removed one leaves it
    const double je = rot ? lr * (col[0] * phi[0] + col[1] * phi[1] + col[2] * phi[2]) : lt * cx * sel3(li - 3, et[0], et[1], et[2]);
    d -= sg * je;
    q_block<S0>(a, rot, li, sg, lr, lt, col, cx, M0, c0);
    q_block<S1>(a, rot, li, sg, lr, lt, col, cx, M1, c1);
    if (S2 >= 0) q_block<(S2 >= 0 ? S2 : 0)>(a, rot, li, sg, lr, lt, col, cx, M2, c2);
}

__global__ void __launch_bounds__(256) k_smooth_cv_query(const CvQueryArgs a) {
    const int lane = threadIdx.x & 63;
    const int64_t q = (int64_t)blockIdx.x * 4 + wave_of_block();   // wave-uniform, as everything below that does not name the lane
    if (q >= a.Q) return;
    const double t = a.qt[q];
    const int F = a.F;
    int lo = 0, hi = F;   // lo -> the number of frames at or before t
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (a.ft[mid] <= t) lo = mid + 1; else hi = mid;
    }
    const int s = lo - 1;
    if (lane == 0) a.seg[q] = s;
    const bool before = s < 0;
    const double te = a.ft[before ? 0 : s];
    if (te == t) {
        // on a frame time: the frame's pose and block, copied
        if (lane < 6) {
            const double v = a.z[6 * (size_t)s + lane];
            a.pose[6 * (size_t)q + lane] = v;
            if (a.start) a.start[6 * (size_t)q + lane] = v;
            if (a.step) a.step[6 * (size_t)q + lane] = 0.0;
        }
        if (a.cov && lane < 36) a.cov[36 * (size_t)q + lane] = a.fc[36 * (size_t)s + lane];
        return;
    }
    const bool after = !before && s == F - 1, inside = !before && !after;
    const int fb = before ? -2 : s - 1;
    // the start pose
    double zm[6];
    if (F == 1) {
        ld6(a.z, zm);
    } else {
        // the motion of the pair (fa, fa + 1), a fraction sc of it applied to the base frame
        const int fa = before ? 0 : after ? F - 2 : s;
        const double D = a.ft[fa + 1] - a.ft[fa];
        const double sc = before ? -((a.ft[0] - t) / D) : (t - te) / D;
        double za[6], zb[6], ra[ENT_STRIDE], rb[ENT_STRIDE], phi[3], et[3];
        ld6(a.z + 6 * (size_t)fa, za);
        ld6(a.z + 6 * (size_t)fa + 6, zb);
        make_ent_row(za, ra);
        make_ent_row(zb, rb);
        pair_terms<false>(ra, rb, nullptr, phi, et, nullptr, nullptr);
        double w[6] = {sc * phi[0], sc * phi[1], sc * phi[2], 0.0, 0.0, 0.0}, ex[ENT_STRIDE], Rb[9], Rm[9], th;
        make_ent_row(w, ex);
#pragma unroll
        for (int i = 0; i < 9; i++) Rb[i] = after ? rb[i] : ra[i];
        mm3(Rb, ex, Rm);
        so3_log(Rm, zm, th);
#pragma unroll
        for (int i = 0; i < 3; i++) zm[3 + i] = (after ? zb[3 + i] : za[3 + i]) + sc * (zb[3 + i] - za[3 + i]);
    }
    // 1. P = Sigma_NN, inverted
    const int r24 = lane < 24 ? lane : 23, r30 = lane < 30 ? lane : 29;
    double A[30];
    {
        const int sl = r24 / 6, li = r24 % 6, f = fb + sl;
        const bool live = f >= 0 && f < F;
#pragma unroll
        for (int c = 0; c < 4; c++) {
            const int g = fb + c, lag = c - sl, al = lag < 0 ? -lag : lag;
            const bool both = live && g >= 0 && g < F;
            const double *blk = (al == 0 ? a.fc : al == 1 ? a.lc : al == 2 ? a.l2 : a.l3) + 36 * (size_t)(both ? (lag >= 0 ? f : g) : 0);
#pragma unroll
            for (int j = 0; j < 6; j++) {
                double v = (c == sl && j == li) ? 1.0 : 0.0;   // a slot without a frame: identity
                if (both) v = blk[lag >= 0 ? 6 * li + j : 6 * j + li];
                A[6 * c + j] = v;
            }
        }
    }
    bool ok = rown_inverse<24>(r24, A);
    // 2. K = P^-1 - F_old, then + F_new, on 30 rows
#pragma unroll
    for (int j = 24; j < 30; j++) A[j] = 0.0;
    if (lane >= 24) {
#pragma unroll
        for (int j = 0; j < 24; j++) A[j] = 0.0;
    }
    double d = 0.0;
    const int slot = r30 / 6, li = r30 % 6;
#pragma unroll 1
    for (int pass = 0; pass < 2; pass++) {
        const double sg = pass ? 1.0 : -1.0;
        // second-difference terms: 0, 1 removed; 2, 3, 4 added
#pragma unroll 1
        for (int k = pass ? 2 : 0; k < (pass ? 5 : 2); k++) {
            const int sp = k == 0 ? 0 : k == 1 ? 1 : k == 2 ? 0 : k == 3 ? 1 : 4;
            const int sc = k == 0 ? 1 : k == 1 ? 2 : k == 2 ? 1 : k == 3 ? 4 : 2;
            const int sn = k == 0 ? 2 : k == 1 ? 3 : k == 2 ? 4 : k == 3 ? 2 : 3;
            const bool lft = (inside && s >= 1) || (k == 2 && after && F >= 2), rgt = (inside && s + 1 <= F - 2) || (k == 4 && before && F >= 2);
            const bool on = (k == 0 || k == 2) ? lft : (k == 1 || k == 4) ? rgt : inside;
            if (!on) continue;
            double zz[6], rp[ENT_STRIDE], rc[ENT_STRIDE], rn[ENT_STRIDE], phi[3], et[3], Mp[9], Mc[9], Mn[9];
            if (sp == 4) {
#pragma unroll
                for (int i = 0; i < 6; i++) zz[i] = zm[i];
            } else {
                ld6(a.z + 6 * (size_t)(fb + sp), zz);
            }
            make_ent_row(zz, rp);
            if (sc == 4) {
#pragma unroll
                for (int i = 0; i < 6; i++) zz[i] = zm[i];
            } else {
                ld6(a.z + 6 * (size_t)(fb + sc), zz);
            }
            make_ent_row(zz, rc);
            if (sn == 4) {
#pragma unroll
                for (int i = 0; i < 6; i++) zz[i] = zm[i];
            } else {
                ld6(a.z + 6 * (size_t)(fb + sn), zz);
            }
            make_ent_row(zz, rn);
            const double tp = sp == 4 ? t : a.ft[fb + sp], tc = sc == 4 ? t : a.ft[fb + sc], tn = sn == 4 ? t : a.ft[fb + sn];
            const double D = tn - tc, r = D / (tc - tp), lr = 1.0 / (a.sr2 * D), lt = 1.0 / (a.st2 * D);
            cv_term<true>(rp, rc, rn, r, phi, et, Mp, Mc, Mn);
            const double cp = r, cc = -(1.0 + r);
            switch (k) {
            case 0: q_acc<0, 1, 2>(A, d, slot, li, sg, lr, lt, phi, et, Mp, cp, Mc, cc, Mn, 1.0); break;
            case 1: q_acc<1, 2, 3>(A, d, slot, li, sg, lr, lt, phi, et, Mp, cp, Mc, cc, Mn, 1.0); break;
            case 2: q_acc<0, 1, 4>(A, d, slot, li, sg, lr, lt, phi, et, Mp, cp, Mc, cc, Mn, 1.0); break;
            case 3: q_acc<1, 4, 2>(A, d, slot, li, sg, lr, lt, phi, et, Mp, cp, Mc, cc, Mn, 1.0); break;
            default: q_acc<4, 2, 3>(A, d, slot, li, sg, lr, lt, phi, et, Mp, cp, Mc, cc, Mn, 1.0); break;
            }
        }
        // pair 0: 0, 1 removed; 2, 3 added
#pragma unroll 1
        for (int k = pass ? 2 : 0; k < (pass ? 4 : 2); k++) {
            const int si = k == 0 ? 1 : k == 1 ? 2 : k == 2 ? 1 : 4, sj = k == 0 ? 2 : k == 1 ? 3 : k == 2 ? 4 : 2;
            const bool on = k == 0 ? inside && s == 0 : k == 1 ? before && F >= 2 : k == 2 ? (inside && s == 0) || (after && F == 1) : before;
            if (!on) continue;
            double zz[6], ri[ENT_STRIDE], rj[ENT_STRIDE], phi[3], et[3], Ma[9], Mb[9];
            if (si == 4) {
#pragma unroll
                for (int i = 0; i < 6; i++) zz[i] = zm[i];
            } else {
                ld6(a.z + 6 * (size_t)(fb + si), zz);
            }
            make_ent_row(zz, ri);
            if (sj == 4) {
#pragma unroll
                for (int i = 0; i < 6; i++) zz[i] = zm[i];
            } else {
                ld6(a.z + 6 * (size_t)(fb + sj), zz);
            }
            make_ent_row(zz, rj);
            const double D = (sj == 4 ? t : a.ft[fb + sj]) - (si == 4 ? t : a.ft[fb + si]);
            const double lr = 1.0 / (a.sr02 * D), lt = 1.0 / (a.st02 * D);
            pair_terms<true>(ri, rj, nullptr, phi, et, Ma, Mb);
            switch (k) {
            case 0: q_acc<1, 2, -1>(A, d, slot, li, sg, lr, lt, phi, et, Ma, -1.0, Mb, 1.0, Mb, 0.0); break;
            case 1: q_acc<2, 3, -1>(A, d, slot, li, sg, lr, lt, phi, et, Ma, -1.0, Mb, 1.0, Mb, 0.0); break;
            case 2: q_acc<1, 4, -1>(A, d, slot, li, sg, lr, lt, phi, et, Ma, -1.0, Mb, 1.0, Mb, 0.0); break;
            default: q_acc<4, 2, -1>(A, d, slot, li, sg, lr, lt, phi, et, Ma, -1.0, Mb, 1.0, Mb, 0.0); break;
            }
        }
    }
    // 3. the neighbours eliminated
    ok = rown_eliminate<30, 24>(r30, A, d) && ok;
    // 4. the 6x6 block of m inverted among lanes 24 .. 29
#pragma unroll
    for (int k = 0; k < 6; k++) {
        double pr[6];
#pragma unroll
        for (int j = 0; j < 6; j++) pr[j] = bc(A[24 + j], 24 + k);
        const double p = pr[k];
        ok = ok && p > 0.0;
        const double ip = 1.0 / p, f = A[24 + k];
        const bool own = r30 == 24 + k;
#pragma unroll
        for (int j = 0; j < 6; j++) {
            const double v = pr[j] * ip;
            if (j != k) A[24 + j] = own ? v : fma(-f, v, A[24 + j]);
        }
        A[24 + k] = own ? ip : -f * ip;
    }
    // the upper triangle from the lower one
#pragma unroll
    for (int i = 0; i < 5; i++)
#pragma unroll
        for (int j = i + 1; j < 6; j++) {
            const double v = bc(A[24 + i], 24 + j);
            if (r30 == 24 + i) A[24 + j] = v;
        }
    double x = 0.0;
#pragma unroll
    for (int j = 0; j < 6; j++) x = fma(A[24 + j], bc(d, 24 + j), x);
    if (!ok && lane == 0) a.flag[0] = 1;
    if (lane >= 24 && lane < 30) {
        const double z0 = li < 3 ? sel3(li, zm[0], zm[1], zm[2]) : sel3(li - 3, zm[3], zm[4], zm[5]);
        a.pose[6 * (size_t)q + li] = z0 + x;
        if (a.start) a.start[6 * (size_t)q + li] = z0;
        if (a.step) a.step[6 * (size_t)q + li] = x;
        if (a.cov) {
#pragma unroll
            for (int j = 0; j < 6; j++) a.cov[36 * (size_t)q + 6 * li + j] = A[24 + j];
        }
    }
}

}  // namespace

// l3 [F - 3][36], l3[f] = (H^-1)_{f,f+3}, from the area launch_smooth_cv_selinv worked on (S at its start, R[0] behind it: the supernode blocks
// after stride 1), on the same stream; a non-positive pivot of an S[k] sets flag[0] = 1.  Returns its launches: none below four frames.
int launch_smooth_cv_lag3(int F, const double *area, double *l3, int32_t *flag, hipStream_t st) {
    if (F < 4) return 0;
    CvLag3Args a;
    a.F = F; a.K = smooth_cv_nodes(F);
    a.S = area; a.R = area + 144 * (size_t)a.K; a.l3 = l3; a.flag = flag;
    hipLaunchKernelGGL(k_cv_lag3, dim3((a.K + 3) / 4), dim3(256), 0, st, a);
    return 1;
}

// The answers of Q queries (Q > 0, F > 0) into pose [Q][6], cov [Q][36] (or NULL) and seg [Q], start and step [Q][6] or NULL, all on the device.
// z [F][6] the frame poses, ft [F] the frame times, qt [Q] the query times; fc, lc, l2 of launch_smooth_cv_selinv at z and l3 of
// launch_smooth_cv_lag3 on the same stream; a non-positive pivot in a query's eliminations sets flag[0] = 1 (the caller zeroes it).  One launch.
int launch_smooth_cv_query(int F, const double *z, const double *ft, double sigma_rot, double sigma_trans, double sigma_rot0, double sigma_trans0,
                           const double *fc, const double *lc, const double *l2, const double *l3, int64_t Q, const double *qt, double *pose,
                           double *cov, double *start, double *step, int32_t *seg, int32_t *flag, hipStream_t st) {
    CvQueryArgs a;
    a.z = z; a.ft = ft; a.fc = fc; a.lc = lc; a.l2 = l2; a.l3 = l3; a.qt = qt; a.pose = pose; a.cov = cov; a.start = start; a.step = step;
    a.seg = seg; a.flag = flag;
    a.sr2 = sigma_rot * sigma_rot; a.st2 = sigma_trans * sigma_trans; a.sr02 = sigma_rot0 * sigma_rot0; a.st02 = sigma_trans0 * sigma_trans0;
    a.F = F; a.Q = Q;
    hipLaunchKernelGGL(k_smooth_cv_query, dim3((unsigned)((Q + 3) / 4)), dim3(256), 0, st, a);
    return 1;
}

}  // namespace aar
