// The smoothed track at any time: pose and 6x6 covariance block at query times that are not frame times, defined as
// what the smoother would report for a frame WITHOUT detections inserted at the query's time.  Inputs are what aar_track_smooth_covariance
// leaves on the device: the frame poses z, S[f] = (H^-1)_ff and R[f] = (H^-1)_{f,f+1} (launch_smooth_selinv), the pairs' lambda.
//
// With F(z_i, z_j, D) = J^T L J the 12x12 information of one between factor (J = [J_a J_b] of section 16, no expected motion), which is
// block diagonal in (rotation, translation):  F_ii = [l_r M_a^T M_a, l_t I],  F_ij = [l_r M_a^T M_b, -l_t I],  F_jj = [l_r M_b^T M_b, l_t I]:
//
//   inside a gap (a, b = a + 1), alpha = (t - t_a) / (t_b - t_a):
//     z_m = (log(R_a Exp(alpha log(R_a^T R_b))), t_a + alpha (t_b - t_a))
//     P^-1 of P = [S_a R_a; R_a^T S_b] by a block Schur complement:   X = S_b - R_a^T S_a^-1 R_a,  W = S_a^-1 R_a,  V = W X^-1
//       P^-1_aa = S_a^-1 + V W^T,   P^-1_ab = -V,   P^-1_bb = X^-1
//     M = P^-1 - F(z_a, z_b, D) + the (a, a) block of F1 = F(z_a, z_m, t - t_a) + the (b, b) block of F2 = F(z_m, z_b, t_b - t)
//     B_a = F1_am,  B_b = F2_mb^T,  C = F1_mm + F2_mm
//     (a, b) eliminated by a second block Schur complement:  G = M_aa^-1 B_a,  Z = M_aa^-1 M_ab,  Y = M_bb - M_ab^T Z,  E = B_b - M_ab^T G
//     cov = (C - B_a^T G - E^T Y^-1 E)^-1
//   outside (end frame e, D = |t - t_e|):  z_m = z_e,  cov = (F_mm - F_me (S_e^-1 + F_ee)^-1 F_em)^-1, the factor taken as (m, e) before the
//     start and (e, m) after the end
//   on a frame time: z_f and S_f copied
//
// k_smooth_query: ONE THREAD PER QUERY, fp64, every loop unrolled over constant indices so that the 6x6 blocks live in registers; five
// spd6_inverse per query inside a gap, three outside.  No atomics, no LDS, nothing shared between queries, a fixed operation order: a query's
// bits depend on nothing but its own time and the track.  A non-positive pivot in any inverse raises the flag with a plain store.  The last
// inverse writes both triangles from one value: the blocks are symmetric to the bit.
#include "geom.hpp"
#include "kernels.h"
#include "pair_terms.hpp"
#include "so3.hpp"

namespace aar {

namespace {

struct QueryArgs {
    const double *z;         // [F][6] frame poses
    const double *ft;        // [F] frame times, ascending
    const double *lam;       // [F-1][2] the pairs' lambda (COV)
    const double *S, *R;     // [F][36] each (COV)
    const double *qt;        // [Q] query times
    double *pose;            // [Q][6]
    double *cov;             // [Q][36] (COV)
    int32_t *seg;            // [Q]
    int32_t *flag;           // raised by a non-positive pivot (COV)
    double sr2, st2;         // sigma_rot^2, sigma_trans^2
    int F;
    int64_t Q;
};

// r = l X^T Y (3x3, row-major)
__device__ __forceinline__ void q_gram(const double *X, const double *Y, double l, double *r) {
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int j = 0; j < 3; j++) r[3 * i + j] = l * (X[i] * Y[j] + X[3 + i] * Y[3 + j] + X[6 + i] * Y[6 + j]);
}

// m (lower triangle) from a row-major symmetric block in memory, inverted
__device__ __forceinline__ bool q_inv_mem(const double *p, double *out) {
    double m[6][6];
#pragma unroll
    for (int i = 0; i < 6; i++)
#pragma unroll
        for (int j = 0; j <= i; j++) m[i][j] = p[6 * i + j];
    return spd6_inverse(m, out);
}

// entry (i, j) of the block-diagonal [r 0; 0 s I]
__device__ __forceinline__ double q_at(const double *r, double s, int i, int j) {
    return (i < 3 && j < 3) ? r[3 * i + j] : (i == j ? s : 0.0);
}

// the inverse of T = [Cr 0; 0 cs I] - B^T Mi B for the coupling B = [br 0; 0 bs I] (rows: the eliminated pose, columns: the new one)
__device__ __forceinline__ bool q_outside(const double *Mi, const double *br, double bs, const double *Cr, double cs, double *out) {
    // G = Mi B
    double G[36];
#pragma unroll
    for (int i = 0; i < 6; i++) {
#pragma unroll
        for (int j = 0; j < 3; j++) G[6 * i + j] = Mi[6 * i] * br[j] + Mi[6 * i + 1] * br[3 + j] + Mi[6 * i + 2] * br[6 + j];
#pragma unroll
        for (int j = 3; j < 6; j++) G[6 * i + j] = Mi[6 * i + j] * bs;
    }
    double T[6][6];
#pragma unroll
    for (int i = 0; i < 6; i++)
#pragma unroll
        for (int j = 0; j <= i; j++) {
            const double u = i < 3 ? br[i] * G[j] + br[3 + i] * G[6 + j] + br[6 + i] * G[12 + j] : bs * G[6 * i + j];
            T[i][j] = q_at(Cr, cs, i, j) - u;
        }
    return spd6_inverse(T, out);
}

template <bool COV>
__global__ void __launch_bounds__(64) k_smooth_query(const QueryArgs a) {
    const int64_t q = (int64_t)blockIdx.x * 64 + threadIdx.x;
    if (q >= a.Q) return;
    const double t = a.qt[q];
    const int F = a.F;
    int lo = 0, hi = F;   // lo -> the number of frames at or before t
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (a.ft[mid] <= t) lo = mid + 1; else hi = mid;
    }
    const int s = lo - 1;
    a.seg[q] = s;
    double *po = a.pose + 6 * (size_t)q;
    double *co = COV ? a.cov + 36 * (size_t)q : nullptr;
    const bool before = s < 0;
    const int e = before ? 0 : s;
    const double te = a.ft[e];
    if (before || s == F - 1 || te == t) {
        // on a frame or outside the sequence: the pose of frame e
        double ze[6];
        ld6(a.z + 6 * (size_t)e, ze);
#pragma unroll
        for (int i = 0; i < 6; i++) po[i] = ze[i];
        if (!COV) return;
        const double *se = a.S + 36 * (size_t)e;
        if (te == t) {
#pragma unroll
            for (int i = 0; i < 36; i++) co[i] = se[i];
            return;
        }
        const double D = fabs(t - te);
        const double lr = 1.0 / (a.sr2 * D), lt = 1.0 / (a.st2 * D);
        double re[ENT_STRIDE], phi[3], et[3], Ma[9], Mb[9];
        make_ent_row(ze, re);
        pair_terms<true>(re, re, nullptr, phi, et, Ma, Mb);
        // before the start the new pose is the factor's a side, after the end its b side
        const double *Mm = before ? Ma : Mb, *Me = before ? Mb : Ma;
        double ee[9], em[9], mm[9];
        q_gram(Me, Me, lr, ee);
        q_gram(Me, Mm, lr, em);
        q_gram(Mm, Mm, lr, mm);
        double I[36];
        bool ok = q_inv_mem(se, I);
        double M[6][6];
#pragma unroll
        for (int i = 0; i < 6; i++)
#pragma unroll
            for (int j = 0; j <= i; j++) M[i][j] = I[6 * i + j] + q_at(ee, lt, i, j);
        ok = spd6_inverse(M, I) && ok;
        double out[36];
        ok = q_outside(I, em, -lt, mm, lt, out) && ok;
        if (!ok) a.flag[0] = 1;
#pragma unroll
        for (int i = 0; i < 36; i++) co[i] = out[i];
        return;
    }
    // inside the gap (s, s + 1)
    const double tb = a.ft[s + 1];
    const double al = (t - te) / (tb - te);
    double za[6], zb[6], zm[6], ra[ENT_STRIDE], rb[ENT_STRIDE], rm[ENT_STRIDE];
    ld6(a.z + 6 * (size_t)s, za);
    ld6(a.z + 6 * (size_t)s + 6, zb);
    make_ent_row(za, ra);
    make_ent_row(zb, rb);
    double phi[3], et[3], Ma0[9], Mb0[9];
    pair_terms<COV>(ra, rb, nullptr, phi, et, Ma0, Mb0);
    {
        // R_m = R_a Exp(alpha phi); its canonical rotation vector
        double w[6] = {al * phi[0], al * phi[1], al * phi[2], 0.0, 0.0, 0.0}, ex[ENT_STRIDE], Rm[9], th;
        make_ent_row(w, ex);
#pragma unroll
        for (int i = 0; i < 3; i++)
#pragma unroll
            for (int j = 0; j < 3; j++) Rm[3 * i + j] = ra[3 * i] * ex[j] + ra[3 * i + 1] * ex[3 + j] + ra[3 * i + 2] * ex[6 + j];
        so3_log(Rm, zm, th);
#pragma unroll
        for (int i = 0; i < 3; i++) zm[3 + i] = za[3 + i] + al * (zb[3 + i] - za[3 + i]);
    }
#pragma unroll
    for (int i = 0; i < 6; i++) po[i] = zm[i];
    if (!COV) return;
    make_ent_row(zm, rm);
    double Ma1[9], Mb1[9], Ma2[9], Mb2[9];
    pair_terms<true>(ra, rm, nullptr, phi, et, Ma1, Mb1);
    pair_terms<true>(rm, rb, nullptr, phi, et, Ma2, Mb2);
    const double lr0 = a.lam[2 * (size_t)s], lt0 = a.lam[2 * (size_t)s + 1];
    const double lr1 = 1.0 / (a.sr2 * (t - te)), lt1 = 1.0 / (a.st2 * (t - te));
    const double lr2 = 1.0 / (a.sr2 * (tb - t)), lt2 = 1.0 / (a.st2 * (tb - t));
    const double *sa = a.S + 36 * (size_t)s, *sb = sa + 36, *rr = a.R + 36 * (size_t)s;
    bool ok = true;
    // P^-1: Ia = S_a^-1, W = Ia R, Xi = (S_b - R^T W)^-1, V = W Xi
    double Ia[36], W[36], Xi[36], V[36];
    ok = q_inv_mem(sa, Ia) && ok;
#pragma unroll
    for (int c = 0; c < 6; c++) {
        double x[6];
#pragma unroll
        for (int k = 0; k < 6; k++) x[k] = rr[6 * k + c];
#pragma unroll
        for (int r = 0; r < 6; r++) {
            double u = 0.0;
#pragma unroll
            for (int k = 0; k < 6; k++) u = fma(Ia[6 * r + k], x[k], u);
            W[6 * r + c] = u;
        }
    }
    {
        double X[6][6];
#pragma unroll
        for (int i = 0; i < 6; i++)
#pragma unroll
            for (int j = 0; j <= i; j++) {
                double u = 0.0;
#pragma unroll
                for (int k = 0; k < 6; k++) u = fma(rr[6 * k + i], W[6 * k + j], u);
                X[i][j] = sb[6 * i + j] - u;
            }
        ok = spd6_inverse(X, Xi) && ok;
    }
#pragma unroll
    for (int i = 0; i < 6; i++)
#pragma unroll
        for (int j = 0; j < 6; j++) {
            double u = 0.0;
#pragma unroll
            for (int k = 0; k < 6; k++) u = fma(W[6 * i + k], Xi[6 * k + j], u);
            V[6 * i + j] = u;
        }
    // M_aa = Ia + V W^T - F0_aa + F1_aa (lower), inverted in place of Ia;  M_ab = -V - F0_ab in V;  M_bb = Xi - F0_bb + F2_bb in Xi
    {
        double f0[9], f1[9], Maa[6][6];
        q_gram(Ma0, Ma0, lr0, f0);
        q_gram(Ma1, Ma1, lr1, f1);
#pragma unroll
        for (int i = 0; i < 6; i++)
#pragma unroll
            for (int j = 0; j <= i; j++) {
                double u = Ia[6 * i + j];
#pragma unroll
                for (int k = 0; k < 6; k++) u = fma(V[6 * i + k], W[6 * j + k], u);
                Maa[i][j] = (u - q_at(f0, lt0, i, j)) + q_at(f1, lt1, i, j);
            }
        ok = spd6_inverse(Maa, Ia) && ok;
    }
    {
        double f0[9], f2[9];
        q_gram(Ma0, Mb0, lr0, f0);
#pragma unroll
        for (int i = 0; i < 6; i++)
#pragma unroll
            for (int j = 0; j < 6; j++) V[6 * i + j] = -V[6 * i + j] - q_at(f0, -lt0, i, j);
        q_gram(Mb0, Mb0, lr0, f0);
        q_gram(Mb2, Mb2, lr2, f2);
#pragma unroll
        for (int i = 0; i < 6; i++)
#pragma unroll
            for (int j = 0; j <= i; j++) Xi[6 * i + j] = (Xi[6 * i + j] - q_at(f0, lt0, i, j)) + q_at(f2, lt2, i, j);
    }
    // Z = M_aa^-1 M_ab in W;  Y = M_bb - M_ab^T Z (lower), inverted into Xi
#pragma unroll
    for (int i = 0; i < 6; i++)
#pragma unroll
        for (int j = 0; j < 6; j++) {
            double u = 0.0;
#pragma unroll
            for (int k = 0; k < 6; k++) u = fma(Ia[6 * i + k], V[6 * k + j], u);
            W[6 * i + j] = u;
        }
    {
        double Y[6][6];
#pragma unroll
        for (int i = 0; i < 6; i++)
#pragma unroll
            for (int j = 0; j <= i; j++) {
                double u = 0.0;
#pragma unroll
                for (int k = 0; k < 6; k++) u = fma(V[6 * k + i], W[6 * k + j], u);
                Y[i][j] = Xi[6 * i + j] - u;
            }
        ok = spd6_inverse(Y, Xi) && ok;
    }
    // G = M_aa^-1 B_a in W, B_a = [ba 0; 0 -lt1 I];  E = B_b - M_ab^T G in Ia, B_b = [bb^T 0; 0 -lt2 I] with bb = l_r2 M_a2^T M_b2 (rows m)
    double ba[9], bb[9];
    q_gram(Ma1, Mb1, lr1, ba);
    q_gram(Ma2, Mb2, lr2, bb);
#pragma unroll
    for (int i = 0; i < 6; i++) {
        double g[6];
#pragma unroll
        for (int j = 0; j < 3; j++) g[j] = Ia[6 * i] * ba[j] + Ia[6 * i + 1] * ba[3 + j] + Ia[6 * i + 2] * ba[6 + j];
#pragma unroll
        for (int j = 3; j < 6; j++) g[j] = -lt1 * Ia[6 * i + j];
#pragma unroll
        for (int j = 0; j < 6; j++) W[6 * i + j] = g[j];
    }
#pragma unroll
    for (int i = 0; i < 6; i++)
#pragma unroll
        for (int j = 0; j < 6; j++) {
            double u = 0.0;
#pragma unroll
            for (int k = 0; k < 6; k++) u = fma(V[6 * k + i], W[6 * k + j], u);
            Ia[6 * i + j] = ((i < 3 && j < 3) ? bb[3 * j + i] : (i == j ? -lt2 : 0.0)) - u;
        }
    // U = Y^-1 E in V;  T = C - B_a^T G - E^T U (lower), C = [l_r1 M_b1^T M_b1 + l_r2 M_a2^T M_a2, (lt1 + lt2) I]
#pragma unroll
    for (int i = 0; i < 6; i++)
#pragma unroll
        for (int j = 0; j < 6; j++) {
            double u = 0.0;
#pragma unroll
            for (int k = 0; k < 6; k++) u = fma(Xi[6 * i + k], Ia[6 * k + j], u);
            V[6 * i + j] = u;
        }
    double out[36];
    {
        double c1[9], c2[9], T[6][6];
        q_gram(Mb1, Mb1, lr1, c1);
        q_gram(Ma2, Ma2, lr2, c2);
#pragma unroll
        for (int i = 0; i < 6; i++)
#pragma unroll
            for (int j = 0; j <= i; j++) {
                const double bg = i < 3 ? ba[i] * W[j] + ba[3 + i] * W[6 + j] + ba[6 + i] * W[12 + j] : -lt1 * W[6 * i + j];
                double u = 0.0;
#pragma unroll
                for (int k = 0; k < 6; k++) u = fma(Ia[6 * k + i], V[6 * k + j], u);
                T[i][j] = ((q_at(c1, lt1, i, j) + q_at(c2, lt2, i, j)) - bg) - u;
            }
        ok = spd6_inverse(T, out) && ok;
    }
    if (!ok) a.flag[0] = 1;
#pragma unroll
    for (int i = 0; i < 36; i++) co[i] = out[i];
}

}  // namespace

// The answers of Q queries (Q > 0, F > 0) into pose [Q][6], cov [Q][36] and seg [Q], all on the device.  z [F][6] the frame poses, ft [F] the
// frame times, qt [Q] the query times.  cov != NULL: after launch_smooth_eval at z, launch_smooth_solve(w, F, 0.0, st) and
// launch_smooth_selinv(w, F, S, R, st) on the same stream; a non-positive pivot in a query's inverses sets flag[0] = 1 (the caller zeroes it).
// cov == NULL: poses and segments only, w, S, R, flag unused.  One launch.
int launch_smooth_query(const SmoothWork &w, int F, const double *z, const double *ft, double sigma_rot, double sigma_trans, const double *S,
                        const double *R, int64_t Q, const double *qt, double *pose, double *cov, int32_t *seg, int32_t *flag, hipStream_t st) {
    QueryArgs a;
    a.z = z; a.ft = ft; a.lam = cov ? w.lam : nullptr; a.S = S; a.R = R; a.qt = qt; a.pose = pose; a.cov = cov; a.seg = seg; a.flag = flag;
    a.sr2 = sigma_rot * sigma_rot; a.st2 = sigma_trans * sigma_trans; a.F = F; a.Q = Q;
    const dim3 grid((unsigned)((Q + 63) / 64));
    if (cov) hipLaunchKernelGGL(k_smooth_query<true>, grid, dim3(64), 0, st, a);
    else hipLaunchKernelGGL(k_smooth_query<false>, grid, dim3(64), 0, st, a);
    return 1;
}

}  // namespace aar
