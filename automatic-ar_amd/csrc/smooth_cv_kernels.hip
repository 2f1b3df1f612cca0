// Smoothed tracking under a constant-velocity prior: the data terms of track() with a second-difference prior,
//
//   E(z) = sum_f E_f(z_f) + e_0^T L_0 e_0 + sum_{1 <= f <= F-2} e_f^T L_f e_f
//   e_0 = between(z_0, z_1)                                        (a random-walk pair with its own sigmas: the prior on the first velocity)
//   e_f = [ log((R_f dR_f)^T R_{f+1})^v ; t_{f+1} - t_f - r_f (t_f - t_{f-1}) ],  dR_f = Exp(r_f log(R_{f-1}^T R_f)),  r_f = dt_f / dt_{f-1}
//
// and one LM over all 6F unknowns.  H is block pentadiagonal.  No atomics anywhere (every sum has one owner and a fixed order):
//   k_smooth_cv_eval<true>   one wavefront per frame: V_f, g_f, E_f by track_eval, then the up to three terms the frame takes part in (and
//                            pair 0) -> H_ff, H_{f,f+1}, H_{f,f+2}, b_f and the cost of the term whose newest frame it is
//   k_smooth_cv_eval<false>  the error-only pass at z + delta, with |delta_f|^2 and delta_f . b_f
//   k_cv_*                   (H + mu I) delta = b: frames paired into supernodes (2k, 2k + 1), 12x12 blocks, block tridiagonal; section 16's
//                            cyclic reduction on them with ONE WAVEFRONT PER SUPERNODE: lane i < 12 keeps row i of every block in registers
//                            and an entry of another row travels through v_readlane, so there is no LDS and no barrier inside a node's work.
//
// Jacobian of term f over (w_{f-1}, w_f, w_{f+1}) (R(w + dw) = Exp(J_l(w) dw) R), psi = log(R_{f-1}^T R_f), Q = (R_f dR)^T R_{f+1}, phi = log Q:
//   d phi / d w_{f+1} = J_r(phi)^-1 J_l(w_{f+1})^T                                  = M_n
//   B = J_r(phi)^-1 Q^T J_r(r psi) J_r(psi)^-1          (phi through dR: d phi = -r J_r(phi)^-1 Q^T J_r(r psi) d psi,
//                                                        d psi = J_r(psi)^-1 R_f^T (theta_f - theta_{f-1}))
//   d phi / d w_f     = -J_r(phi)^-1 R_{f+1}^T J_l(w_f) - r B J_l(w_f)^T            = M_c
//   d phi / d w_{f-1} = r B R_f^T J_l(w_{f-1})                                      = M_p
//   the translation rows are (r, -(1 + r), 1) I.
#include <algorithm>
#include "cv_rows.hpp"
#include "cv_term.hpp"
#include "geom.hpp"
#include "kernels.h"
#include "pair_terms.hpp"
#include "so3.hpp"
#include "track_eval.hpp"

namespace aar {

namespace {

struct SmoothCvArgs {
    TrackArgs t;            // the data term (t.z, t.iters_out, t.err_out unused)
    SmoothCvWork w;
    const double *z;        // [F][6] the point
    const double *delta;    // error-only pass: evaluate at z + delta ...
    double *zt;             // ... and leave that point here
    double *Ef, *Pe;        // [F] data cost per frame, [F] prior cost per term
};

// the entity row of frame g at the point of this pass
template <bool WITH_J>
__device__ __forceinline__ void cv_row(const SmoothCvArgs &a, int g, double *row) {
    double z[6];
    ld6(a.z + 6 * (size_t)g, z);
    if (!WITH_J) {
#pragma unroll
        for (int i = 0; i < 6; i++) z[i] += a.delta[6 * (size_t)g + i];
    }
    make_ent_row(z, row);
}

// what the prior adds to a frame's blocks: a 3x3 rotation block and a multiple of I on the translations
struct CvAcc {
    double Dr[9], O1r[9], O2r[9], br[3], bt[3], dt, o1t, o2t;
};
__device__ __forceinline__ void acc_mtm(double *Z, double l, const double *X, const double *Y) {   // Z += l X^T Y
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int j = 0; j < 3; j++) Z[3 * i + j] += l * (X[i] * Y[j] + X[3 + i] * Y[3 + j] + X[6 + i] * Y[6 + j]);
}
// the frame's own part of one term: Jacobian [Mx 0; 0 cx I], then the couplings to the one and two frames after it
__device__ __forceinline__ void cv_add(CvAcc &q, double lr, double lt, const double *phi, const double *et, const double *Mx, double cx,
                                       const double *My, double cy, const double *Mz, double cz) {
    acc_mtm(q.Dr, lr, Mx, Mx);
    q.dt += lt * cx * cx;
#pragma unroll
    for (int i = 0; i < 3; i++) {
        q.br[i] -= lr * (Mx[i] * phi[0] + Mx[3 + i] * phi[1] + Mx[6 + i] * phi[2]);
        q.bt[i] -= lt * cx * et[i];
    }
    if (My) { acc_mtm(q.O1r, lr, Mx, My); q.o1t += lt * cx * cy; }
    if (Mz) { acc_mtm(q.O2r, lr, Mx, Mz); q.o2t += lt * cx * cz; }
}

template <bool WITH_J>
__global__ void __launch_bounds__(256) k_smooth_cv_eval(const SmoothCvArgs a) {
    const int lane = threadIdx.x & 63, f = blockIdx.x * 4 + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);   // wave-uniform
    const int F = a.t.F;
    if (f >= F) return;
    double zc[6];
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
        if (lane < 6) a.zt[6 * (size_t)f + lane] = a.z[6 * (size_t)f + lane] + a.delta[6 * (size_t)f + lane];
        if (lane == 0) { a.w.lin[2 * (size_t)f] = d2; a.w.lin[2 * (size_t)f + 1] = dg; }
    }
    double V[21], g[6];
    const double Ef = track_eval<WITH_J>(a.t, f, zc, lane, V, g);
    CvAcc q;
#pragma unroll
    for (int i = 0; i < 9; i++) q.Dr[i] = q.O1r[i] = q.O2r[i] = 0.0;
#pragma unroll
    for (int i = 0; i < 3; i++) q.br[i] = q.bt[i] = 0.0;
    q.dt = q.o1t = q.o2t = 0.0;
    double Pe = 0.0;   // of the term whose newest frame this is: term f - 1 (pair 0 for frame 1)
    // pair 0
    if (f <= 1 && F > 1 && (WITH_J || f == 1)) {
        double ra[ENT_STRIDE], rb[ENT_STRIDE], phi[3], et[3], Ma[9], Mb[9];
        cv_row<WITH_J>(a, 0, ra);
        cv_row<WITH_J>(a, 1, rb);
        pair_terms<WITH_J>(ra, rb, nullptr, phi, et, Ma, Mb);
        const double lr = a.w.lam[0], lt = a.w.lam[1];
        if (f == 1) Pe = lr * (phi[0] * phi[0] + phi[1] * phi[1] + phi[2] * phi[2]) + lt * (et[0] * et[0] + et[1] * et[1] + et[2] * et[2]);
        if (WITH_J) {
            if (f == 0) cv_add(q, lr, lt, phi, et, Ma, -1.0, Mb, 1.0, nullptr, 0.0);
            else cv_add(q, lr, lt, phi, et, Mb, 1.0, nullptr, 0.0, nullptr, 0.0);
        }
    }
    // the terms centred on f - 1, f, f + 1 (the error-only pass needs the first alone)
#pragma unroll 1
    for (int k = 0; k < (WITH_J ? 3 : 1); k++) {
        const int c = f - 1 + k;
        if (c < 1 || c > F - 2) continue;
        double rp[ENT_STRIDE], rc[ENT_STRIDE], rn[ENT_STRIDE], phi[3], et[3], Mp[9], Mc[9], Mn[9];
        cv_row<WITH_J>(a, c - 1, rp);
        cv_row<WITH_J>(a, c, rc);
        cv_row<WITH_J>(a, c + 1, rn);
        const double r = a.w.ratio[c], lr = a.w.lam[2 * (size_t)c], lt = a.w.lam[2 * (size_t)c + 1];
        cv_term<WITH_J>(rp, rc, rn, r, phi, et, Mp, Mc, Mn);
        if (k == 0) Pe = lr * (phi[0] * phi[0] + phi[1] * phi[1] + phi[2] * phi[2]) + lt * (et[0] * et[0] + et[1] * et[1] + et[2] * et[2]);
        if (WITH_J) {
            if (k == 0) cv_add(q, lr, lt, phi, et, Mn, 1.0, nullptr, 0.0, nullptr, 0.0);
            else if (k == 1) cv_add(q, lr, lt, phi, et, Mc, -(1.0 + r), Mn, 1.0, nullptr, 0.0);
            else cv_add(q, lr, lt, phi, et, Mp, r, Mc, -(1.0 + r), Mn, 1.0);
        }
    }
    if (lane == 0) {
        a.Ef[f] = Ef;
        if (f > 0) a.Pe[f - 1] = Pe;
        else a.Pe[F - 1] = 0.0;
        if (WITH_J) {
            double *d = a.w.Dg + 36 * (size_t)f, *o1 = a.w.O1 + 36 * (size_t)f, *o2 = a.w.O2 + 36 * (size_t)f, *b = a.w.rhs + 6 * (size_t)f;
#pragma unroll
            for (int i = 0; i < 6; i++) {
                b[i] = g[i] + (i < 3 ? q.br[i] : q.bt[i - 3]);   // track_eval's g is already -J^T r_w
#pragma unroll
                for (int j = 0; j < 6; j++) {
                    const bool rr = i < 3 && j < 3, tt = i >= 3 && i == j;
                    d[6 * i + j] = V[sym6(i, j)] + (rr ? q.Dr[3 * i + j] : tt ? q.dt : 0.0);
                    o1[6 * i + j] = rr ? q.O1r[3 * i + j] : tt ? q.o1t : 0.0;
                    o2[6 * i + j] = rr ? q.O2r[3 * i + j] : tt ? q.o2t : 0.0;
                }
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------------------------
// Block cyclic reduction on the supernodes.  The scheme, the in-place ownership rule and what is kept for the back-substitution are those of
// smooth_kernels.hip: supernode k carries D_k (12x12), U_k (its coupling to the next active supernode on the right) and b_k; at stride s the
// even multiples of s eliminate their neighbours at +-s, rewriting only their own D, U, b and reading only odd supernodes besides; Dinv[r]
// and Ls[r] (the coupling from the left neighbour) are kept when r is eliminated.
//
// One wavefront works on one supernode.  Lane i < 12 holds row i of a block in twelve registers (lanes 12..63 repeat lane 11 and store
// nothing); row p of another operand reaches every lane through v_readlane, so a product is 144 broadcasts and 144 fma per lane, every sum
// in ascending p.  Transposes cost nothing: a lane loads column i instead of row i.
// The row helpers live in cv_rows.hpp, shared with the selected inverse (smooth_cv_cov_kernels.hip).
// ---------------------------------------------------------------------------------------------------------------------------------
struct CvCrArgs {
    SmoothCvWork w;
    int F, K;
    double mu;
};

// supernode k from the frames' blocks, damped; a frame past the end is an identity block with a zero right-hand side
__device__ __forceinline__ void cv_damp(const CvCrArgs &a, int k, int lane) {
    if (lane < 12) {
        const int F = a.F, fa = 2 * k, fr = fa + lane / 6, li = lane % 6;   // this row's frame and its row there
        double *dw = a.w.Dw + 144 * (size_t)k + 12 * lane, *uw = a.w.Uw + 144 * (size_t)k + 12 * lane;
        const bool live = fr < F;
        for (int j = 0; j < 12; j++) {
            const int fc = fa + j / 6, lj = j % 6;   // the column's frame within the supernode
            double d = 0.0;
            if (live && fc < F) {
                if (fc == fr) d = a.w.Dg[36 * (size_t)fr + 6 * li + lj] + (li == lj ? a.mu : 0.0);
                else if (fc > fr) d = a.w.O1[36 * (size_t)fr + 6 * li + lj];
                else d = a.w.O1[36 * (size_t)fc + 6 * lj + li];
            } else if (fc == fr && li == lj) {
                d = 1.0;
            }
            dw[j] = d;
            // the coupling to supernode k + 1: frames fa + 2, fa + 3
            const int fu = fa + 2 + j / 6, lag = fu - fr;   // 1, 2 or 3
            double u = 0.0;
            if (live && fu < F) {
                if (lag == 1) u = a.w.O1[36 * (size_t)fr + 6 * li + lj];
                else if (lag == 2) u = a.w.O2[36 * (size_t)fr + 6 * li + lj];
            }
            uw[j] = u;
        }
        a.w.bw[12 * (size_t)k + lane] = live ? a.w.rhs[6 * (size_t)fr + li] : 0.0;
    }
    if (k == 0 && lane == 0) a.w.flag[0] = 0;
}

// even supernode j at stride s (j a multiple of 2 s) eliminates j + s and j - s
__device__ __forceinline__ void cv_eliminate(const CvCrArgs &a, int j, int s, int lane) {
    const int K = a.K, ri = lane < 12 ? lane : 11;
    double D[12];
    ld_row(a.w.Dw + 144 * (size_t)j, ri, D);
    double b = a.w.bw[12 * (size_t)j + ri];
    bool ok = true;
    if (j + s < K) {
        const int r = j + s;
        double I[12], U[12], Ut[12], T[12];
        ld_row(a.w.Dw + 144 * (size_t)r, ri, I);
        ld_row(a.w.Uw + 144 * (size_t)j, ri, U);
        ld_col(a.w.Uw + 144 * (size_t)j, ri, Ut);
        const double br = a.w.bw[12 * (size_t)r + ri];
        ok = row_inverse(ri, I) && ok;
        // T = U D_r^-1;  D -= T U^T;  b -= T b_r;  U' = -T U_r
        row_mm<false>(U, I, 1.0, T);
        row_mm<true>(T, Ut, -1.0, D);
        b -= row_mv(T, br);
        st_row(a.w.Dinv + 144 * (size_t)r, lane, I);
        st_row(a.w.Ls + 144 * (size_t)r, lane, U);
        if (r + s < K) {
            double Ur[12], Un[12];
            ld_row(a.w.Uw + 144 * (size_t)r, ri, Ur);
            row_mm<false>(T, Ur, -1.0, Un);
            st_row(a.w.Uw + 144 * (size_t)j, lane, Un);
        }
    }
    if (j - s >= 0) {
        const int q = j - s;
        double I[12], Lq[12], Lt[12], T[12];
        ld_row(a.w.Dw + 144 * (size_t)q, ri, I);
        ld_row(a.w.Uw + 144 * (size_t)q, ri, Lq);   // rows: supernode q, columns: supernode j
        ld_col(a.w.Uw + 144 * (size_t)q, ri, Lt);
        const double bq = a.w.bw[12 * (size_t)q + ri];
        ok = row_inverse(ri, I) && ok;
        // T = Lq^T D_q^-1;  D -= T Lq;  b -= T b_q
        row_mm<false>(Lt, I, 1.0, T);
        row_mm<true>(T, Lq, -1.0, D);
        b -= row_mv(T, bq);
    }
    st_row(a.w.Dw + 144 * (size_t)j, lane, D);
    if (lane < 12) a.w.bw[12 * (size_t)j + lane] = b;
    if (!ok && lane == 0) a.w.flag[0] = 1;
}

__device__ __forceinline__ void cv_root(const CvCrArgs &a, int lane) {
    const int ri = lane < 12 ? lane : 11;
    double I[12];
    ld_row(a.w.Dw, ri, I);
    const double b = a.w.bw[ri];
    const bool ok = row_inverse(ri, I);
    const double x = row_mv(I, b);
    if (lane < 12) a.w.delta[lane] = x;
    if (!ok && lane == 0) a.w.flag[0] = 1;
}

// eliminated supernode i (an odd multiple of s): x_i = D_i^-1 (b_i - Ls_i^T x_{i-s} - U_i x_{i+s})
__device__ __forceinline__ void cv_backsub(const CvCrArgs &a, int i, int s, int lane) {
    const int ri = lane < 12 ? lane : 11;
    double M[12];
    double v = a.w.bw[12 * (size_t)i + ri];
    ld_col(a.w.Ls + 144 * (size_t)i, ri, M);
    v -= row_mv(M, a.w.delta[12 * (size_t)(i - s) + ri]);
    if (i + s < a.K) {
        ld_row(a.w.Uw + 144 * (size_t)i, ri, M);
        v -= row_mv(M, a.w.delta[12 * (size_t)(i + s) + ri]);
    }
    ld_row(a.w.Dinv + 144 * (size_t)i, ri, M);
    const double x = row_mv(M, v);
    if (lane < 12) a.w.delta[12 * (size_t)i + lane] = x;
}

__global__ void __launch_bounds__(256) k_cv_damp(const CvCrArgs a) {
    const int k = blockIdx.x * 4 + wave_of_block();
    if (k < a.K) cv_damp(a, k, threadIdx.x & 63);
}

__global__ void __launch_bounds__(256) k_cv_level(const CvCrArgs a, int s) {
    const int64_t j = (int64_t)(blockIdx.x * 4 + wave_of_block()) * 2 * s;
    if (j < a.K) cv_eliminate(a, (int)j, s, threadIdx.x & 63);
}

__global__ void __launch_bounds__(256) k_cv_back(const CvCrArgs a, int s) {
    const int64_t i = (int64_t)(blockIdx.x * 4 + wave_of_block()) * 2 * s + s;
    if (i < a.K) cv_backsub(a, (int)i, s, threadIdx.x & 63);
}

// one workgroup of four wavefronts: (damping when it starts at the finest level,) every elimination level from stride s0 up, the root, and
// the back-substitution down to s0.  A wavefront takes the supernodes wv, wv + 4, ... of a level; the barriers stand BETWEEN the levels,
// outside those loops, and the level loops run on K and s0 alone, so every wavefront meets every barrier the same number of times.
__global__ void __launch_bounds__(256) k_cv_tail(const CvCrArgs a, int s0) {
    const int lane = threadIdx.x & 63, wv = wave_of_block(), K = a.K;
    if (s0 == 1) {
        for (int k = wv; k < K; k += 4) cv_damp(a, k, lane);
        __syncthreads();
    }
    int s = s0;
    for (; s < K; s *= 2) {
        for (int64_t j = (int64_t)wv * 2 * s; j < K; j += (int64_t)8 * s) cv_eliminate(a, (int)j, s, lane);
        __syncthreads();
    }
    if (wv == 0) cv_root(a, lane);
    __syncthreads();
    for (s /= 2; s >= s0; s /= 2) {
        for (int64_t i = (int64_t)wv * 2 * s + s; i < K; i += (int64_t)8 * s) cv_backsub(a, (int)i, s, lane);
        __syncthreads();
    }
}

SmoothCvArgs cv_eval_args(const DeviceProblem &P, int which, const SmoothCvWork &w) {
    SmoothCvArgs a;
    a.t.idx = P.a_idx; a.t.uv = P.a_uv; a.t.ent = P.ent[which]; a.t.frame_obs_start = P.frame_obs_start;
    { const KTable kt = k_table(P, which); a.t.Kmat = kt.base; a.t.kstride = kt.stride; }
    a.t.A = P.A; a.t.F = P.F; a.t.huber = P.huber; a.t.h = P.half_size;
    a.t.max_iters = 0; a.t.min_error = a.t.min_step_error_diff = a.t.min_average_step_error_diff = a.t.tau = 0.0;
    a.t.z = nullptr; a.t.iters_out = nullptr; a.t.err_out = nullptr;
    a.w = w;
    return a;
}

}  // namespace

size_t smooth_cv_work_doubles(int F) {
    const size_t n = (size_t)std::max(F, 1), k = (size_t)smooth_cv_nodes((int)n);
    return n * (2 * 6 + 3 * 36 + 6 + 4 + 2 + 2 + 1) + k * (12 + 4 * 144 + 12) + 8 + 2;
}

void smooth_cv_work_carve(SmoothCvWork &w, double *base, int F) {
    const size_t n = (size_t)std::max(F, 1), k = (size_t)smooth_cv_nodes((int)n);
    double *p = base;
    auto take = [&](size_t c) { double *q = p; p += c; return q; };
    w.z[0] = take(6 * n); w.z[1] = take(6 * n); w.delta = take(12 * k);
    w.Dg = take(36 * n); w.O1 = take(36 * n); w.O2 = take(36 * n);
    w.Dw = take(144 * k); w.Uw = take(144 * k); w.Dinv = take(144 * k); w.Ls = take(144 * k);
    w.rhs = take(6 * n); w.bw = take(12 * k);
    w.Ef[0] = take(n); w.Ef[1] = take(n); w.Pe[0] = take(n); w.Pe[1] = take(n);
    w.lin = take(2 * n); w.lam = take(2 * n); w.ratio = take(n);
    w.res = take(8);
    w.flag = reinterpret_cast<int32_t *>(take(2));
}

// H, b and the costs at z[cur] (with_j), or the costs at z[cur] + delta -> z[1 - cur] with the linear model's sums; then the reduction into w.res
void launch_smooth_cv_eval(const DeviceProblem &P, int which, const SmoothCvWork &w, int cur, bool with_j, hipStream_t st) {
    if (P.F == 0) return;
    SmoothCvArgs a = cv_eval_args(P, which, w);
    a.z = w.z[cur];
    const int out = with_j ? cur : 1 - cur;
    a.delta = with_j ? nullptr : w.delta;
    a.zt = with_j ? nullptr : w.z[1 - cur];
    a.Ef = w.Ef[out]; a.Pe = w.Pe[out];
    if (with_j) hipLaunchKernelGGL(k_smooth_cv_eval<true>, dim3((P.F + 3) / 4), dim3(256), 0, st, a);
    else hipLaunchKernelGGL(k_smooth_cv_eval<false>, dim3((P.F + 3) / 4), dim3(256), 0, st, a);
    launch_smooth_reduce(w.Ef[out], w.Pe[out], with_j ? nullptr : w.lin, with_j ? w.Dg : nullptr, w.flag, P.F, w.res, st);
}

// damping, the own levels, the tail, the own levels' back-substitutions; the tail alone when it starts at the finest level
int smooth_cv_solve_launches(int F) {
    if (F == 0) return 0;
    const int n = cv_own_levels(smooth_cv_nodes(F));
    return n ? 2 * n + 2 : 1;
}

// (H + mu I) delta = rhs; returns the number of launches
int launch_smooth_cv_solve(const SmoothCvWork &w, int F, double mu, hipStream_t st) {
    if (F == 0) return 0;
    CvCrArgs a;
    a.w = w; a.F = F; a.K = smooth_cv_nodes(F); a.mu = mu;
    const int K = a.K, n = cv_own_levels(K);
    if (n) hipLaunchKernelGGL(k_cv_damp, dim3((K + 3) / 4), dim3(256), 0, st, a);
    for (int l = 0; l < n; l++) hipLaunchKernelGGL(k_cv_level, dim3((cv_evens(K, 1 << l) + 3) / 4), dim3(256), 0, st, a, 1 << l);
    hipLaunchKernelGGL(k_cv_tail, dim3(1), dim3(256), 0, st, a, 1 << n);
    for (int l = n - 1; l >= 0; l--) hipLaunchKernelGGL(k_cv_back, dim3((cv_evens(K, 1 << l) + 3) / 4), dim3(256), 0, st, a, 1 << l);
    return smooth_cv_solve_launches(F);
}

}  // namespace aar
