// Smoothed tracking: the frames' data terms of track() tied together by a motion prior between consecutive frames,
//
//   E(z) = sum_f E_f(z_f) + sum_{f < F-1} e_f^T L_f e_f,   e_f = [ log((R_f dR_f)^T R_{f+1})^v ; t_{f+1} - t_f - dt_f ],  L_f = diag(lr x3, lt x3)
//
// and one LM over all 6F unknowns.  Three kinds of kernels, no atomics anywhere (every sum has one owner and a fixed order):
//   k_smooth_eval<true>    one wavefront per frame: V_f, g_f, E_f by track_eval, then the between factors of pairs f-1 and f on top -> the
//                          diagonal block H_ff, the off-diagonal block H_{f,f+1}, the right-hand side, the pair's cost
//   k_smooth_eval<false>   the error-only pass at z + delta (the trial point), with the linear model's |delta|^2 and delta.b per frame
//   k_smooth_reduce        one workgroup: the sums (and the largest diagonal entry) in a fixed order -> one 8-double record the host reads
//   k_cr_*                 (H + mu I) delta = b by block cyclic (odd-even) reduction on the 6x6 blocks: at stride s the nodes that are even
//                          multiples of s eliminate their neighbours at +-s.  One launch per level while a level has more nodes than one
//                          workgroup has threads, then ONE workgroup finishes the elimination, solves the root and substitutes back down to
//                          the level it started from; the remaining back-substitution levels are one launch each.
//
// With J_a, J_b the Jacobians of e_f over (w_f, t_f) and (w_{f+1}, t_{f+1}) (R(w + dw) = Exp(J_l(w) dw) R):
//   Q = (R_f dR)^T R_{f+1},  phi = log(Q)^v
//   d phi / d w_{f+1} = J_r(phi)^-1 J_l(w_{f+1})^T                = M_b      (Q' = Q Exp(R_{f+1}^T J_l(w_{f+1}) dw), R^T J_l = J_l^T = J_r)
//   d phi / d w_f     = -J_r(phi)^-1 R_{f+1}^T J_l(w_f)           = M_a      (Q' = Q Exp(-R_{f+1}^T J_l(w_f) dw))
//   J_a = [M_a 0; 0 -I],  J_b = [M_b 0; 0 I]
#include <algorithm>
#include "geom.hpp"
#include "kernels.h"
#include "pair_terms.hpp"
#include "so3.hpp"
#include "track_eval.hpp"

namespace aar {

namespace {

struct SmoothArgs {
    TrackArgs t;            // the data term (t.z, t.iters_out, t.err_out unused)
    SmoothWork w;
    const double *z;        // [F][6] the point
    const double *delta;    // error-only pass: evaluate at z + delta ...
    double *zt;             // ... and leave that point here
    double *Ef, *Pe;        // [F] data cost per frame, [F] prior cost per pair (entry F-1 = 0)
};

template <bool WITH_J>
__global__ void __launch_bounds__(256) k_smooth_eval(const SmoothArgs a) {
    const int lane = threadIdx.x & 63, f = blockIdx.x * 4 + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);   // wave-uniform
    const int F = a.t.F;
    if (f >= F) return;
    // the poses of frames f - 1, f, f + 1 (every lane the same values)
    double zc[6], rowc[ENT_STRIDE];
    ld6(a.z + 6 * (size_t)f, zc);
    if (!WITH_J) {
        double d[6];
        ld6(a.delta + 6 * (size_t)f, d);
        double d2 = 0.0, dg = 0.0;
#pragma unroll
        for (int i = 0; i < 6; i++) {
            zc[i] += d[i];
            d2 += d[i] * d[i];
            dg += d[i] * a.w.rhs[6 * (size_t)f + i];
        }
        if (lane < 6) a.zt[6 * (size_t)f + lane] = a.z[6 * (size_t)f + lane] + a.delta[6 * (size_t)f + lane];   // (the same sum, without indexing registers)
        if (lane == 0) { a.w.lin[2 * (size_t)f] = d2; a.w.lin[2 * (size_t)f + 1] = dg; }
    }
    make_ent_row(zc, rowc);
    double V[21], g[6];
    const double Ef = track_eval<WITH_J>(a.t, f, zc, lane, V, g);
    double D[6][6], b[6];
    if (WITH_J) {
#pragma unroll
        for (int i = 0; i < 6; i++) {
            b[i] = g[i];   // track_eval's g is already -J^T r_w
#pragma unroll
            for (int j = 0; j < 6; j++) D[i][j] = V[sym6(i, j)];
        }
    }
    // pair f - 1: this frame is its b side (its cost belongs to frame f - 1)
    if (WITH_J && f > 0) {
        double zp[6], rowp[ENT_STRIDE];
        ld6(a.z + 6 * (size_t)(f - 1), zp);
        make_ent_row(zp, rowp);
        double phi[3], et[3], Ma[9], Mb[9];
        pair_terms<true>(rowp, rowc, a.w.rel ? a.w.rel + 6 * (size_t)(f - 1) : nullptr, phi, et, Ma, Mb);
        const double lr = a.w.lam[2 * (size_t)(f - 1)], lt = a.w.lam[2 * (size_t)(f - 1) + 1];
#pragma unroll
        for (int i = 0; i < 3; i++) {
#pragma unroll
            for (int j = 0; j < 3; j++) D[i][j] += lr * (Mb[i] * Mb[j] + Mb[3 + i] * Mb[3 + j] + Mb[6 + i] * Mb[6 + j]);
            D[3 + i][3 + i] += lt;
            b[i] -= lr * (Mb[i] * phi[0] + Mb[3 + i] * phi[1] + Mb[6 + i] * phi[2]);
            b[3 + i] -= lt * et[i];
        }
    }
    double Pe = 0.0;
    if (f + 1 < F) {
        double zn[6], rown[ENT_STRIDE];
        ld6(a.z + 6 * (size_t)(f + 1), zn);
        if (!WITH_J) {
#pragma unroll
            for (int i = 0; i < 6; i++) zn[i] += a.delta[6 * (size_t)(f + 1) + i];
        }
        make_ent_row(zn, rown);
        double phi[3], et[3], Ma[9], Mb[9];
        pair_terms<WITH_J>(rowc, rown, a.w.rel ? a.w.rel + 6 * (size_t)f : nullptr, phi, et, Ma, Mb);
        const double lr = a.w.lam[2 * (size_t)f], lt = a.w.lam[2 * (size_t)f + 1];
        Pe = lr * (phi[0] * phi[0] + phi[1] * phi[1] + phi[2] * phi[2]) + lt * (et[0] * et[0] + et[1] * et[1] + et[2] * et[2]);
        if (WITH_J) {
            double O[36];
#pragma unroll
            for (int i = 0; i < 36; i++) O[i] = 0.0;
#pragma unroll
            for (int i = 0; i < 3; i++) {
#pragma unroll
                for (int j = 0; j < 3; j++) {
                    D[i][j] += lr * (Ma[i] * Ma[j] + Ma[3 + i] * Ma[3 + j] + Ma[6 + i] * Ma[6 + j]);
                    O[6 * i + j] = lr * (Ma[i] * Mb[j] + Ma[3 + i] * Mb[3 + j] + Ma[6 + i] * Mb[6 + j]);
                }
                D[3 + i][3 + i] += lt;
                O[6 * (3 + i) + 3 + i] = -lt;
                b[i] -= lr * (Ma[i] * phi[0] + Ma[3 + i] * phi[1] + Ma[6 + i] * phi[2]);
                b[3 + i] += lt * et[i];
            }
            if (lane == 0) {
                double *o = a.w.Of + 36 * (size_t)f;
#pragma unroll
                for (int i = 0; i < 36; i++) o[i] = O[i];
            }
        }
    }
    if (lane == 0) {
        a.Ef[f] = Ef;
        a.Pe[f] = Pe;
        if (WITH_J) {
            double *d = a.w.Dg + 36 * (size_t)f, *r = a.w.rhs + 6 * (size_t)f;
#pragma unroll
            for (int i = 0; i < 6; i++) {
                r[i] = b[i];
#pragma unroll
                for (int j = 0; j < 6; j++) d[6 * i + j] = D[i][j];
            }
        }
    }
}

// res[0] = sum E_f, [1] = sum of the pairs' costs, [2] = |delta|^2, [3] = delta . b, [4] = max diagonal of H, [5] = the solve's pivot flag.
// Thread t adds entries t, t + 256, ... ascending, then a fixed tree over the 256 partial sums.
__global__ void __launch_bounds__(256) k_smooth_reduce(const double *Ef, const double *Pe, const double *lin, const double *Dg, const int32_t *flag,
                                                       int F, double *res) {
    __shared__ double sh[5][256];
    const int t = threadIdx.x;
    double s[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
    for (int f = t; f < F; f += 256) {
        s[0] += Ef[f];
        s[1] += Pe[f];
        if (lin) { s[2] += lin[2 * (size_t)f]; s[3] += lin[2 * (size_t)f + 1]; }
        if (Dg) {
#pragma unroll
            for (int i = 0; i < 6; i++) s[4] = fmax(s[4], Dg[36 * (size_t)f + 7 * i]);
        }
    }
#pragma unroll
    for (int q = 0; q < 5; q++) sh[q][t] = s[q];
    __syncthreads();
    for (int off = 128; off > 0; off >>= 1) {
        if (t < off) {
#pragma unroll
            for (int q = 0; q < 4; q++) sh[q][t] += sh[q][t + off];
            sh[4][t] = fmax(sh[4][t], sh[4][t + off]);
        }
        __syncthreads();
    }
    if (t < 5) res[t] = sh[t][0];
    if (t == 5) res[5] = (double)flag[0];
    if (t == 6) res[6] = 0.0;
    if (t == 7) res[7] = 0.0;
}

// ---------------------------------------------------------------------------------------------------------------------------------
// Block cyclic reduction.  Node i carries D_i (diagonal block), U_i (its coupling to the next active node on the right; the coupling to the
// left is the left neighbour's U transposed) and b_i.  At stride s the active nodes are the multiples of s; those that are odd multiples
// are eliminated by their even neighbours.  Everything happens in place: an even node rewrites only its own D, U, b and reads only odd
// nodes besides, which nobody writes at that level.  What the back-substitution of an eliminated node r needs later is kept when it is
// eliminated: Dinv[r] and Ls[r] = the coupling from its left neighbour (which that neighbour is about to overwrite); its own U_r and b_r are
// never touched again.
// ---------------------------------------------------------------------------------------------------------------------------------
struct CrArgs {
    SmoothWork w;
    int F;
    double mu;
};

__device__ __forceinline__ void ld36(const double *p, double *m) {
#pragma unroll
    for (int i = 0; i < 36; i++) m[i] = p[i];
}
__device__ __forceinline__ bool inv_block(const double *p, double *inv) {
    double m[6][6];
#pragma unroll
    for (int i = 0; i < 6; i++)
#pragma unroll
        for (int j = 0; j < 6; j++) m[i][j] = p[6 * i + j];
    return spd6_inverse(m, inv);
}

__device__ __forceinline__ void cr_damp(const CrArgs &a, int f) {
    const double *d = a.w.Dg + 36 * (size_t)f, *o = a.w.Of + 36 * (size_t)f;
    double *dw = a.w.Dw + 36 * (size_t)f, *uw = a.w.Uw + 36 * (size_t)f;
    const bool has_u = f + 1 < a.F;
#pragma unroll
    for (int i = 0; i < 36; i++) {
        dw[i] = d[i] + ((i % 7) == 0 ? a.mu : 0.0);
        uw[i] = has_u ? o[i] : 0.0;
    }
#pragma unroll
    for (int i = 0; i < 6; i++) a.w.bw[6 * (size_t)f + i] = a.w.rhs[6 * (size_t)f + i];
    if (f == 0) a.w.flag[0] = 0;
}

// even node j at stride s (j a multiple of 2 s) eliminates j + s and j - s
__device__ __forceinline__ void cr_eliminate(const CrArgs &a, int j, int s) {
    const int F = a.F;
    double D[36], b[6];
    ld36(a.w.Dw + 36 * (size_t)j, D);
    ld6(a.w.bw + 6 * (size_t)j, b);
    bool ok = true;
    if (j + s < F) {
        const int r = j + s;
        double I[36], U[36], T[36];
        ok = inv_block(a.w.Dw + 36 * (size_t)r, I) && ok;
        ld36(a.w.Uw + 36 * (size_t)j, U);
        double *dinv = a.w.Dinv + 36 * (size_t)r, *ls = a.w.Ls + 36 * (size_t)r;
#pragma unroll
        for (int i = 0; i < 36; i++) { dinv[i] = I[i]; ls[i] = U[i]; }
        // T = U D_r^-1;  D -= T U^T (lower triangle, mirrored);  b -= T b_r;  U' = -T U_r
#pragma unroll
        for (int i = 0; i < 6; i++)
#pragma unroll
            for (int k = 0; k < 6; k++) {
                double t = 0.0;
#pragma unroll
                for (int p = 0; p < 6; p++) t = fma(U[6 * i + p], I[6 * p + k], t);
                T[6 * i + k] = t;
            }
#pragma unroll
        for (int i = 0; i < 6; i++)
#pragma unroll
            for (int k = 0; k <= i; k++) {
                double t = 0.0;
#pragma unroll
                for (int p = 0; p < 6; p++) t = fma(T[6 * i + p], U[6 * k + p], t);
                D[6 * i + k] -= t;
                if (k != i) D[6 * k + i] = D[6 * i + k];
            }
        double br[6];
        ld6(a.w.bw + 6 * (size_t)r, br);
#pragma unroll
        for (int i = 0; i < 6; i++) {
            double t = 0.0;
#pragma unroll
            for (int p = 0; p < 6; p++) t = fma(T[6 * i + p], br[p], t);
            b[i] -= t;
        }
        if (r + s < F) {
            double Ur[36];
            ld36(a.w.Uw + 36 * (size_t)r, Ur);
            double *uo = a.w.Uw + 36 * (size_t)j;
#pragma unroll
            for (int i = 0; i < 6; i++)
#pragma unroll
                for (int k = 0; k < 6; k++) {
                    double t = 0.0;
#pragma unroll
                    for (int p = 0; p < 6; p++) t = fma(T[6 * i + p], Ur[6 * p + k], t);
                    uo[6 * i + k] = -t;
                }
        }
    }
    if (j - s >= 0) {
        const int q = j - s;
        double I[36], Lq[36], T[36];
        ok = inv_block(a.w.Dw + 36 * (size_t)q, I) && ok;
        ld36(a.w.Uw + 36 * (size_t)q, Lq);   // rows: node q, columns: node j
        // T = Lq^T D_q^-1;  D -= T Lq;  b -= T b_q
#pragma unroll
        for (int i = 0; i < 6; i++)
#pragma unroll
            for (int k = 0; k < 6; k++) {
                double t = 0.0;
#pragma unroll
                for (int p = 0; p < 6; p++) t = fma(Lq[6 * p + i], I[6 * p + k], t);
                T[6 * i + k] = t;
            }
#pragma unroll
        for (int i = 0; i < 6; i++)
#pragma unroll
            for (int k = 0; k <= i; k++) {
                double t = 0.0;
#pragma unroll
                for (int p = 0; p < 6; p++) t = fma(T[6 * i + p], Lq[6 * p + k], t);
                D[6 * i + k] -= t;
                if (k != i) D[6 * k + i] = D[6 * i + k];
            }
        double bq[6];
        ld6(a.w.bw + 6 * (size_t)q, bq);
#pragma unroll
        for (int i = 0; i < 6; i++) {
            double t = 0.0;
#pragma unroll
            for (int p = 0; p < 6; p++) t = fma(T[6 * i + p], bq[p], t);
            b[i] -= t;
        }
    }
    double *dw = a.w.Dw + 36 * (size_t)j;
#pragma unroll
    for (int i = 0; i < 36; i++) dw[i] = D[i];
#pragma unroll
    for (int i = 0; i < 6; i++) a.w.bw[6 * (size_t)j + i] = b[i];
    if (!ok) a.w.flag[0] = 1;
}

__device__ __forceinline__ void cr_root(const CrArgs &a) {
    double I[36], b[6];
    if (!inv_block(a.w.Dw, I)) a.w.flag[0] = 1;
    ld6(a.w.bw, b);
#pragma unroll
    for (int i = 0; i < 6; i++) {
        double t = 0.0;
#pragma unroll
        for (int p = 0; p < 6; p++) t = fma(I[6 * i + p], b[p], t);
        a.w.delta[i] = t;
    }
}

// eliminated node i (an odd multiple of s): x_i = D_i^-1 (b_i - Ls_i^T x_{i-s} - U_i x_{i+s})
__device__ __forceinline__ void cr_backsub(const CrArgs &a, int i, int s) {
    double v[6], x[6], M[36];
    ld6(a.w.bw + 6 * (size_t)i, v);
    ld6(a.w.delta + 6 * (size_t)(i - s), x);
    ld36(a.w.Ls + 36 * (size_t)i, M);
#pragma unroll
    for (int r = 0; r < 6; r++) {
        double t = 0.0;
#pragma unroll
        for (int p = 0; p < 6; p++) t = fma(M[6 * p + r], x[p], t);
        v[r] -= t;
    }
    if (i + s < a.F) {
        ld6(a.w.delta + 6 * (size_t)(i + s), x);
        ld36(a.w.Uw + 36 * (size_t)i, M);
#pragma unroll
        for (int r = 0; r < 6; r++) {
            double t = 0.0;
#pragma unroll
            for (int p = 0; p < 6; p++) t = fma(M[6 * r + p], x[p], t);
            v[r] -= t;
        }
    }
    ld36(a.w.Dinv + 36 * (size_t)i, M);
#pragma unroll
    for (int r = 0; r < 6; r++) {
        double t = 0.0;
#pragma unroll
        for (int p = 0; p < 6; p++) t = fma(M[6 * r + p], v[p], t);
        a.w.delta[6 * (size_t)i + r] = t;
    }
}

__global__ void __launch_bounds__(64) k_cr_damp(const CrArgs a) {
    const int f = blockIdx.x * 64 + threadIdx.x;
    if (f < a.F) cr_damp(a, f);
}

__global__ void __launch_bounds__(64) k_cr_level(const CrArgs a, int s) {
    const int64_t j = (int64_t)(blockIdx.x * 64 + threadIdx.x) * 2 * s;
    if (j < a.F) cr_eliminate(a, (int)j, s);
}

__global__ void __launch_bounds__(64) k_cr_back(const CrArgs a, int s) {
    const int64_t i = (int64_t)(blockIdx.x * 64 + threadIdx.x) * 2 * s + s;
    if (i < a.F) cr_backsub(a, (int)i, s);
}

// one workgroup: (damping when it starts at the finest level,) every elimination level from stride s0 up, the root, and the
// back-substitution down to s0.  The levels are separated by workgroup barriers; all traffic is through global memory.
__global__ void __launch_bounds__(SMOOTH_TAIL) k_cr_tail(const CrArgs a, int s0) {
    const int t = threadIdx.x, F = a.F;
    if (s0 == 1) {
        for (int f = t; f < F; f += SMOOTH_TAIL) cr_damp(a, f);
        __syncthreads();
    }
    int s = s0;
    for (; s < F; s *= 2) {
        for (int64_t j = (int64_t)t * 2 * s; j < F; j += (int64_t)SMOOTH_TAIL * 2 * s) cr_eliminate(a, (int)j, s);
        __syncthreads();
    }
    if (t == 0) cr_root(a);
    __syncthreads();
    for (s /= 2; s >= s0; s /= 2) {
        for (int64_t i = (int64_t)t * 2 * s + s; i < F; i += (int64_t)SMOOTH_TAIL * 2 * s) cr_backsub(a, (int)i, s);
        __syncthreads();
    }
}

SmoothArgs eval_args(const DeviceProblem &P, int which, const SmoothWork &w) {
    SmoothArgs a;
    a.t.idx = P.a_idx; a.t.uv = P.a_uv; a.t.ent = P.ent[which]; a.t.frame_obs_start = P.frame_obs_start;
    { const KTable kt = k_table(P, which); a.t.Kmat = kt.base; a.t.kstride = kt.stride; }
    a.t.A = P.A; a.t.F = P.F; a.t.huber = P.huber; a.t.h = P.half_size;
    a.t.max_iters = 0; a.t.min_error = a.t.min_step_error_diff = a.t.min_average_step_error_diff = a.t.tau = 0.0;
    a.t.z = nullptr; a.t.iters_out = nullptr; a.t.err_out = nullptr;
    a.w = w;
    return a;
}

}  // namespace

size_t smooth_work_doubles(int F) {
    const size_t n = (size_t)std::max(F, 1);
    return n * (3 * 6 + 6 * 36 + 2 * 6 + 4 + 2 + 2 + 6) + 8 + 2;
}

void smooth_work_carve(SmoothWork &w, double *base, int F) {
    const size_t n = (size_t)std::max(F, 1);
    double *p = base;
    auto take = [&](size_t k) { double *q = p; p += k; return q; };
    w.z[0] = take(6 * n); w.z[1] = take(6 * n); w.delta = take(6 * n);
    w.Dg = take(36 * n); w.Of = take(36 * n); w.Dw = take(36 * n); w.Uw = take(36 * n); w.Dinv = take(36 * n); w.Ls = take(36 * n);
    w.rhs = take(6 * n); w.bw = take(6 * n);
    w.Ef[0] = take(n); w.Ef[1] = take(n); w.Pe[0] = take(n); w.Pe[1] = take(n);
    w.lin = take(2 * n); w.lam = take(2 * n); w.rel_buf = take(6 * n);
    w.res = take(8);
    w.flag = reinterpret_cast<int32_t *>(take(2));
    w.rel = nullptr;
}

// H, b and the costs at z[cur] (with_j), or the costs at z[cur] + delta -> z[1 - cur] with the linear model's sums; then the reduction into w.res
void launch_smooth_eval(const DeviceProblem &P, int which, const SmoothWork &w, int cur, bool with_j, hipStream_t st) {
    if (P.F == 0) return;
    SmoothArgs a = eval_args(P, which, w);
    a.z = w.z[cur];
    const int out = with_j ? cur : 1 - cur;
    a.delta = with_j ? nullptr : w.delta;
    a.zt = with_j ? nullptr : w.z[1 - cur];
    a.Ef = w.Ef[out]; a.Pe = w.Pe[out];
    if (with_j) hipLaunchKernelGGL(k_smooth_eval<true>, dim3((P.F + 3) / 4), dim3(256), 0, st, a);
    else hipLaunchKernelGGL(k_smooth_eval<false>, dim3((P.F + 3) / 4), dim3(256), 0, st, a);
    hipLaunchKernelGGL(k_smooth_reduce, dim3(1), dim3(256), 0, st, (const double *)w.Ef[out], (const double *)w.Pe[out],
                       with_j ? (const double *)nullptr : (const double *)w.lin, with_j ? (const double *)w.Dg : (const double *)nullptr,
                       (const int32_t *)w.flag, P.F, w.res);
}

// the reduction alone, for the evaluation of another prior (smooth_cv_kernels.hip)
void launch_smooth_reduce(const double *Ef, const double *Pe, const double *lin, const double *Dg, const int32_t *flag, int F, double *res,
                          hipStream_t st) {
    hipLaunchKernelGGL(k_smooth_reduce, dim3(1), dim3(256), 0, st, Ef, Pe, lin, Dg, flag, F, res);
}

// (H + mu I) delta = rhs; returns the number of launches
int launch_smooth_solve(const SmoothWork &w, int F, double mu, hipStream_t st) {
    if (F == 0) return 0;
    CrArgs a;
    a.w = w; a.F = F; a.mu = mu;
    int launches = 0, s = 1;
    auto evens = [&](int stride) { return (F + 2 * stride - 1) / (2 * stride); };
    if (evens(1) > SMOOTH_TAIL) {
        hipLaunchKernelGGL(k_cr_damp, dim3((F + 63) / 64), dim3(64), 0, st, a);
        launches++;
        for (; s < F && evens(s) > SMOOTH_TAIL; s *= 2) {
            hipLaunchKernelGGL(k_cr_level, dim3((evens(s) + 63) / 64), dim3(64), 0, st, a, s);
            launches++;
        }
    }
    const int s0 = s;
    hipLaunchKernelGGL(k_cr_tail, dim3(1), dim3(SMOOTH_TAIL), 0, st, a, s0);
    launches++;
    for (s = s0 / 2; s >= 1; s /= 2) {
        hipLaunchKernelGGL(k_cr_back, dim3((evens(s) + 63) / 64), dim3(64), 0, st, a, s);
        launches++;
    }
    return launches;
}

}  // namespace aar
