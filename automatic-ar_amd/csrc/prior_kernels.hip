// Pose priors: one 6x6 block and one 6-vector per prior, added to the reduced system that pass B has built.
//
//   phi = log(R_p^T R)^v,  e = [phi ; t - t_p],  cost = e^T L e,  J = [J_r(phi)^-1 J_r(w)  0 ; 0  I]  (over the entity's z entries (w, t))
//
// J_r(w) = J_l(w)^T, and J_l is the third piece of the entity's {R, t, J_l} row (geom.hpp): R(w + dw) = Exp(J_l dw) R = R Exp(J_r dw).
// One workgroup, one prior per thread (thread t takes priors t, t + 256, ...): e, J, J^T L J, J^T L e and e^T L e are ~600 fp64 operations on
// registers only.  No two priors share an entity (validated on the host), so the diagonal blocks are read-modify-written with plain stores;
// the cost is summed in prior order by wavefront 0 after a barrier.  fp64 throughout.
#include "geom.hpp"
#include "kernels.h"
#include "so3.hpp"

namespace aar {

namespace {

constexpr int PRIOR_THREADS = 256;

struct PriorArgs {
    const int32_t *ent_of;    // [n] shared entity of each prior
    const double *dat;        // [n][PRIOR_DAT]: x6 | info (row-major)
    const double *ent;        // {R, t, J_l} rows of the point
    int n, n_pad;
    int add;                  // 1: add into S / g0 and write the cost into err_slot (rank 0 of an LM problem)
    double *S, *g0, *err_slot;
    double *out;              // [n][8]: e (6) | cost | 0, then [n * 8] = the summed cost
};

// e and J (the 3 x 3 rotation block M; the rest of J is the identity / zero) of prior p at the entity row
__device__ __forceinline__ void prior_terms(const PriorArgs a, int p, double e[6], double M[9], double Lam[36]) {
    const int ent = a.ent_of[p];
    const double *dat = a.dat + (size_t)p * PRIOR_DAT;
    Ent cur;
    load_ent(a.ent, ent, cur);
    double rp[ENT_STRIDE];
    make_ent_row(dat, rp);   // R_p by the Rodrigues formula of every other entity row
    double Q[9];             // R_p^T R
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int j = 0; j < 3; j++) Q[3 * i + j] = rp[i] * cur.R[j] + rp[3 + i] * cur.R[3 + j] + rp[6 + i] * cur.R[6 + j];
    double phi[3], th;
    so3_log(Q, phi, th);
    double Ji[9];
    so3_jr_inv(phi, th, Ji);
    // M = J_r(phi)^-1 J_l(w)^T
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int j = 0; j < 3; j++) M[3 * i + j] = Ji[3 * i] * cur.Jl[3 * j] + Ji[3 * i + 1] * cur.Jl[3 * j + 1] + Ji[3 * i + 2] * cur.Jl[3 * j + 2];
    e[0] = phi[0]; e[1] = phi[1]; e[2] = phi[2];
    e[3] = cur.t[0] - dat[3]; e[4] = cur.t[1] - dat[4]; e[5] = cur.t[2] - dat[5];
#pragma unroll
    for (int i = 0; i < 36; i++) Lam[i] = dat[6 + i];
}

__global__ void __launch_bounds__(PRIOR_THREADS) k_prior(const PriorArgs a) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    for (int p = tid; p < a.n; p += PRIOR_THREADS) {   // one prior per thread: every index below is a compile-time constant (no scratch)
        double e[6], M[9], Lam[36];
        prior_terms(a, p, e, M, Lam);
        const int ent = a.ent_of[p];
        // L J (J = [M 0; 0 I]) and L e
        double LJ[36], Le[6];
#pragma unroll
        for (int r = 0; r < 6; r++) {
#pragma unroll
            for (int j = 0; j < 3; j++) LJ[6 * r + j] = Lam[6 * r] * M[j] + Lam[6 * r + 1] * M[3 + j] + Lam[6 * r + 2] * M[6 + j];
#pragma unroll
            for (int j = 3; j < 6; j++) LJ[6 * r + j] = Lam[6 * r + j];
            double s = 0.0;
#pragma unroll
            for (int c = 0; c < 6; c++) s += Lam[6 * r + c] * e[c];
            Le[r] = s;
        }
        double cost = 0.0;
#pragma unroll
        for (int r = 0; r < 6; r++) cost += e[r] * Le[r];
        if (a.add) {
            // J^T L J, lower triangle of the diagonal block (what pass B writes and every reader reads); B += -J^T L e
            double *S = a.S + (size_t)(6 * ent) * a.n_pad + 6 * ent;
#pragma unroll
            for (int i = 0; i < 6; i++) {
#pragma unroll
                for (int j = 0; j <= i; j++) {
                    const double h = i < 3 ? M[i] * LJ[j] + M[3 + i] * LJ[6 + j] + M[6 + i] * LJ[12 + j] : LJ[6 * i + j];
                    S[(size_t)i * a.n_pad + j] += h;
                }
                const double g = i < 3 ? M[i] * Le[0] + M[3 + i] * Le[1] + M[6 + i] * Le[2] : Le[i];
                a.g0[6 * ent + i] -= g;
            }
        }
        double *o = a.out + (size_t)p * 8;
#pragma unroll
        for (int i = 0; i < 6; i++) o[i] = e[i];
        o[6] = cost;
        o[7] = 0.0;
    }
    __syncthreads();
    if (wave != 0) return;
    // the summed cost in a fixed order: lane l adds priors l, l + 64, ... ascending, then a fixed xor tree
    double s = 0.0;
    for (int p = lane; p < a.n; p += 64) s += a.out[(size_t)p * 8 + 6];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off);
    if (lane == 0) {
        a.out[(size_t)a.n * 8] = s;
        if (a.add) *a.err_slot = s;
    }
}

}  // namespace

void launch_prior(const DeviceProblem &P, int which, bool add, hipStream_t st) {
    if (P.n_prior == 0) return;
    PriorArgs a;
    a.ent_of = P.prior_ent; a.dat = P.prior_dat; a.ent = P.ent[which]; a.n = P.n_prior; a.n_pad = P.n_pad;
    a.add = (add && P.prior_rank0) ? 1 : 0;
    a.S = P.blk[which].S; a.g0 = P.blk[which].g0; a.err_slot = P.err_part + P.F;
    a.out = P.prior_out;
    HookScope _h(P, KID_PRIOR);
    hipLaunchKernelGGL(k_prior, dim3(1), dim3(PRIOR_THREADS), 0, st, a);
}

}  // namespace aar
