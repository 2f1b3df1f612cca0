// Predicted corners, leverages, leave-one-out residuals and the gate on a SMOOTHED track (aar_track_smooth_predict_corners,
// _detection_leverage, _detection_loo, _gate_detections): one 6 x 6 block of the smoother's H^-1 pushed through the projection per query.
// See DESIGN.md section 38.
//
//   k_smooth_corners<MODE>  eight lanes per query, eight queries per wavefront: lanes 8g .. 8g+7 own query 8 wave + g, lane r of the group
//                           owns row r of everything.  Lanes 2k and 2k+1 both project corner k (no exchange) and keep row r of
//                           G = du/dz_f (8 x 6, the smoother's own frame Jacobian, unweighted), row r of T = G Sigma (six terms in index
//                           order) and row r of C = T G^T (six terms, the other rows of G by shuffles inside the group).  The entries
//                           r <= s are then handed to lane s: every pair (r, s), (s, r) is one value.  Modes 3 and 4 run section 37's
//                           tail on registers: A = I - C (3) or I + C (4) with "lane i, register j" where k_predict_corners has sA[i][j] --
//                           the same right-looking Cholesky factorisation, the same two substitutions, r^T w and w^T C w in the same
//                           order -- every exchange a shuffle of width 8 with a static register index.
// No LDS, no atomics, no scratch, fp64 throughout; every sum has one owner and an index order.  No lane leaves before its group's last
// exchange: a bad pivot, a corner behind the camera and a group past n set a predicate and run on (a group past n on query n - 1), only
// the stores are masked.  A query's bits depend on its own inputs alone: its place in the launch and its neighbours do not enter.
#include "geom.hpp"
#include "kernels.h"

namespace aar {

namespace {

// one of eight registers by a lane-dependent index: a chain of selects, no scratch
__device__ __forceinline__ double pick8(int r, double v0, double v1, double v2, double v3, double v4, double v5, double v6, double v7) {
    double o = v0;
    o = r == 1 ? v1 : o; o = r == 2 ? v2 : o; o = r == 3 ? v3 : o; o = r == 4 ? v4 : o;
    o = r == 5 ? v5 : o; o = r == 6 ? v6 : o; o = r == 7 ? v7 : o;
    return o;
}

}  // namespace

// The modes are k_predict_corners': 0 = uv | cov | status, 1 = uv | status (nothing of the chain is read), 2 = trace and diagonal of C of
// the problem's own detections, 3 = their leave-one-out quantities, 4 = the gate of candidate detections.
template <int MODE>
__global__ void __launch_bounds__(64) k_smooth_corners(const SmoothCornersArgs a) {
    const int lane = threadIdx.x, r = lane & 7, gbase = lane & ~7;
    const int64_t q0 = (int64_t)blockIdx.x * 8 + (lane >> 3);
    const bool live = q0 < a.n;
    const int64_t q = live ? q0 : a.n - 1;
    int c, em;
    int64_t ix;   // which pose and which block
    if (MODE == 2 || MODE == 3) {
        const ObsIdx o = a.obs[q];
        c = o.cam; em = o.marker; ix = o.frame;
    } else {
        c = a.q_cam[q]; em = a.C + a.q_marker[q]; ix = q;
    }
    Ent ec, emk, ef;
    load_ent(a.ent, c, ec);
    load_ent(a.ent, em, emk);
    {
        double zf[6], row[ENT_STRIDE];
#pragma unroll
        for (int i = 0; i < 6; i++) zf[i] = a.pose[6 * ix + i];
        make_ent_row(zf, row);   // (as the smoother's own evaluation builds the frame's row: track_eval.hpp)
#pragma unroll
        for (int i = 0; i < 9; i++) { ef.R[i] = row[i]; ef.Jl[i] = row[12 + i]; }
#pragma unroll
        for (int i = 0; i < 3; i++) ef.t[i] = row[9 + i];
    }
    const double *K = a.K + (size_t)a.kstride * c;
    CornerGeom g;
    project_corner(ec, emk, ef, K, a.h, r >> 1, g);
    const double u = (r & 1) ? g.v : g.u;
    const unsigned long long bal = __ballot(!(g.pc[2] > 0.0));
    const bool behind = ((bal >> gbase) & 0xffull) != 0;
    const double nan = __builtin_nan("");
    if (MODE < 2) {
        if (live) a.uv[q * 8 + r] = behind ? nan : u;
        if (MODE == 1) {
            if (live && r == 0) a.status[q] = (uint8_t)(behind ? 1 : 0);
            return;   // (no exchange lies behind this point in this instance)
        }
    }
    // row r of G, of T = G Sigma and of C = T G^T
    double G[6], T[6], Cr[8];
    {
        double Gc[2][6], Gm[2][6], Gf[2][6];
        corner_jacobian<false, false, true>(ec, emk, ef, K, g, Gc, Gm, Gf);
#pragma unroll
        for (int j = 0; j < 6; j++) G[j] = (r & 1) ? Gf[1][j] : Gf[0][j];
    }
    {
        const double *__restrict__ S = a.block + 36 * ix;
#pragma unroll
        for (int j = 0; j < 6; j++) {
            double v = 0.0;
#pragma unroll
            for (int i = 0; i < 6; i++) v = fma(G[i], S[i * 6 + j], v);
            T[j] = v;
        }
    }
#pragma unroll
    for (int s = 0; s < 8; s++) {
        double v = 0.0;
#pragma unroll
        for (int j = 0; j < 6; j++) v = fma(T[j], __shfl(G[j], s, 8), v);
        Cr[s] = v;
    }
    // the entry (i, j), i < j, is lane i's: lane j takes it for its (j, i)
#pragma unroll
    for (int i = 0; i < 8; i++)
#pragma unroll
        for (int j = i + 1; j < 8; j++) {
            const double v = __shfl(Cr[j], i, 8);
            Cr[i] = r == j ? v : Cr[i];
        }
    if (MODE == 0) {
        if (live) {
#pragma unroll
            for (int s = 0; s < 8; s++) a.cov[q * 64 + r * 8 + s] = behind ? nan : Cr[s];
            if (r == 0) a.status[q] = (uint8_t)(behind ? 1 : 0);
        }
        return;
    }
    // the diagonal in every lane, its sum in k_predict_corners' order
    const double dr = pick8(r, Cr[0], Cr[1], Cr[2], Cr[3], Cr[4], Cr[5], Cr[6], Cr[7]);
    double dg[8];
#pragma unroll
    for (int k = 0; k < 8; k++) dg[k] = __shfl(dr, k, 8);
    const double trace = ((dg[0] + dg[1]) + (dg[2] + dg[3])) + ((dg[4] + dg[5]) + (dg[6] + dg[7]));
    if (MODE == 2) {
        if (live) {
            if (a.row_lev) a.row_lev[q * 8 + r] = behind ? nan : dr;
            if (r == 0) { a.lev[q] = behind ? nan : trace; a.status[q] = (uint8_t)(behind ? 1 : 0); }
        }
        return;
    }
    // A = I -+ C: lane i holds row i from here to the end of the factorisation; the innovation
    double Ar[8];
#pragma unroll
    for (int s = 0; s < 8; s++) Ar[s] = MODE == 3 ? (r == s ? 1.0 - Cr[s] : -Cr[s]) : (r == s ? 1.0 + Cr[s] : Cr[s]);
    const double Rr = (double)a.obs_uv[q * 8 + r] - u;
    // A = L L^T, right-looking, column by column; Ld[k] the root of pivot k, the same in every lane.  A bad pivot ends the search for the
    // margin and raises `bad`; the arithmetic runs on and its results are not stored
    double Ld[8], margin = __builtin_inf();
    bool bad = false;
#pragma unroll
    for (int k = 0; k < 8; k++) {
        const double d = __shfl(Ar[k], k, 8);
        if (!bad) {
            if (!(d >= margin)) margin = d;
            if (!(d > PREDICT_LOO_MIN_PIVOT) || !(d < __builtin_inf())) bad = true;
        }
        const double l = sqrt(d);
        Ld[k] = l;
        if (r > k) Ar[k] = Ar[k] / l;
#pragma unroll
        for (int j = k + 1; j < 8; j++) {
            const double ljk = __shfl(Ar[k], j, 8);
            if (r >= j) Ar[j] = fma(-Ar[k], ljk, Ar[j]);
        }
    }
    // L y = r: lane c holds the finished sum of row c when column c is taken away from the rows below
    double y[8], w[8];
    {
        double v = Rr;
#pragma unroll
        for (int cc = 0; cc < 8; cc++) {
            y[cc] = __shfl(v / Ld[cc], cc, 8);
            if (r > cc) v = fma(-Ar[cc], y[cc], v);
        }
    }
    // L^T w = y, every lane the whole of it: row rr loses L[c2][rr] w[c2] for c2 = 7 .. rr + 1, in that order
#pragma unroll
    for (int c2 = 7; c2 >= 0; c2--) {
        w[c2] = y[c2] / Ld[c2];
#pragma unroll
        for (int rr = 0; rr < c2; rr++) y[rr] = fma(-__shfl(Ar[rr], c2, 8), w[c2], y[rr]);
    }
    double qv = 0.0, kv = 0.0;
#pragma unroll
    for (int rr = 0; rr < 8; rr++) qv = fma(__shfl(Rr, rr, 8), w[rr], qv);
    if (MODE == 3) {
        double t = 0.0;
#pragma unroll
        for (int c2 = 0; c2 < 8; c2++) t = fma(Cr[c2], w[c2], t);
#pragma unroll
        for (int rr = 0; rr < 8; rr++) kv = fma(w[rr], __shfl(t, rr, 8), kv);
    }
    if (!live) return;
    const bool none = behind || bad;
    a.loo_w[q * 8 + r] = MODE == 3 ? (none ? nan : pick8(r, w[0], w[1], w[2], w[3], w[4], w[5], w[6], w[7])) : (behind ? nan : Rr);
    if (r != 0) return;
    a.status[q] = (uint8_t)(behind ? 1 : (bad ? PREDICT_UNDETERMINED : 0));
    a.loo_q[q] = none ? nan : qv;
    a.loo_margin[q] = behind ? nan : margin;
    if (MODE == 3) {
        // the scalars of the statistic from the chain's record, as the host forms them for the report
        const double cost = a.res[0] + a.res[1];
        const double sigma2 = a.dof > 0 ? cost / (double)a.dof : 0.0;
        double Fv = nan;
        if (!none && a.dof > 8) {
            const double den = (cost - qv) / (double)(a.dof - 8);
            Fv = den <= 0.0 ? __builtin_inf() : (qv / 8.0) / den;
        }
        a.lev[q] = behind ? nan : trace;
        a.loo_F[q] = Fv;
        a.loo_cook[q] = none ? nan : kv / (a.num_vars * sigma2);
        a.loo_keep[q] = (a.f_max > 0.0 && !none && Fv > a.f_max) ? 0 : 1;
    }
}

void launch_smooth_corners(const SmoothCornersArgs &a, int mode, hipStream_t st) {
    if (a.n <= 0) return;
    const dim3 grid((unsigned)((a.n + 7) / 8)), block(64);
    if (mode == 0) hipLaunchKernelGGL(k_smooth_corners<0>, grid, block, 0, st, a);
    else if (mode == 1) hipLaunchKernelGGL(k_smooth_corners<1>, grid, block, 0, st, a);
    else if (mode == 2) hipLaunchKernelGGL(k_smooth_corners<2>, grid, block, 0, st, a);
    else if (mode == 3) hipLaunchKernelGGL(k_smooth_corners<3>, grid, block, 0, st, a);
    else hipLaunchKernelGGL(k_smooth_corners<4>, grid, block, 0, st, a);
}

}  // namespace aar
