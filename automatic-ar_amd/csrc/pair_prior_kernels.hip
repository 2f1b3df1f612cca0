// Relative pose priors between two cameras or two markers: the first terms that put camera-camera and marker-marker
// blocks into U.  With (R_a, t_a), (R_b, t_b) the entities' poses and (R_rel, t_rel) the prior for T_a^-1 T_b:
//
//   R_ab = R_a^T R_b,  t_ab = R_a^T (t_b - t_a),  phi = log(R_rel^T R_ab)^v,  e = [phi ; t_ab - t_rel],  cost = e^T L e
//   J_a = [ -J_r(phi)^-1 R_b^T J_l(w_a)   0 ;  R_a^T [t_b - t_a]x J_l(w_a)   -R_a^T ]      J_b = [ J_r(phi)^-1 R_b^T J_l(w_b)   0 ;  0   R_a^T ]
//
// over the z entries (w, t) of the two entities (R(w + dw) = Exp(J_l dw) R, J_l from the entity rows).
//
// One workgroup, two phases.  Phase 1, one pair per thread (thread t takes pairs t, t + 256, ...): e, J_a, J_b and the products with L on
// registers only, every index a compile-time constant.  The cross block J_hi^T L J_lo is unique to the pair (validated on the host) and is
// read-modify-written in place; the two diagonal contributions (21 + 6 values a side) go into the pair's record of the workspace.  Phase 2,
// behind a barrier: an entity may be an end of several pairs (a board as a star or a chain), so every free entity that has pairs gets ONE
// writer per value of its diagonal block and its part of g0 -- 27 threads, each summing its value over the entity's (pair, side) list in
// ascending pair order (built on the host) and adding the sum with one plain store.  No atomics; the cost is summed in pair order by
// wavefront 0 with a fixed tree.  A fixed end (root, switched-off group, fixed index) has no list, and a pair with one has no cross block:
// nothing is written to a fixed entity's rows.  fp64 throughout.
//
// Up to PAIR_LDS_MAX pairs the records, the lists and the costs live in LDS (59 KB) and the global workspace is not touched: phase 2 is a chain
// of dependent reads (entity -> items -> records), about 30 ns a link there and about a microsecond in global memory.  Either way a thread
// takes its entities four at a time and has the four values of S / g0 it will add to in flight while it sums.  More pairs: the same code on the
// global arrays.  Both instances add in the same order, so they give the same bits.
#include "geom.hpp"
#include "kernels.h"
#include "so3.hpp"

namespace aar {

namespace {

constexpr int PAIR_THREADS = 256;
constexpr int PAIR_SIDE = 27;              // a side's record: the lower triangle of J^T L J (21, row-major) | J^T L e (6)
constexpr int PAIR_REC = 2 * PAIR_SIDE;    // a | b
constexpr int PAIR_LDS_MAX = 128;          // pairs whose records fit LDS: 128 x 432 B = 54 KB (+ 5 KB of lists and costs) of the 64 KB a launch gets unasked

struct PairPriorArgs {
    const int32_t *ends;      // [n][4]: entity a, entity b, 1 = both ends free (the cross block exists), 0
    const double *dat;        // [n][PRIOR_DAT]: x6_rel | info (row-major)
    const double *ent;        // {R, t, J_l} rows of the point
    const int32_t *el_ent;    // [n_el] the free entities that are an end of a pair, ascending
    const int32_t *el_start;  // [n_el + 1] into el_item
    const int32_t *el_item;   // 2 * pair + side (0 = a, 1 = b), ascending per entity
    int n, n_el, n_items, n_pad;
    int add;                  // 1: add into S / g0 and the cost into err_slot (rank 0 of an LM problem)
    int err_acc;              // 1: k_prior has written err_slot in front of this launch: add to it
    double *S, *g0, *err_slot;
    double *rec;              // [n][PAIR_REC] workspace between the two phases
    double *out;              // [n][8]: e (6) | cost | 0, then [n * 8] = the summed cost
};

// lower triangle of J^T (L J) and J^T (L e) of one side into its record.  J = [N 0; T G] (3 x 3 pieces, row-major)
__device__ __forceinline__ void side_record(const double *N, const double *T, const double *G, const double *LJ, const double *Le, double *rec) {
    int k = 0;
#pragma unroll
    for (int i = 0; i < 6; i++) {
#pragma unroll
        for (int j = 0; j <= i; j++) {
            double h;
            if (i < 3) h = N[i] * LJ[j] + N[3 + i] * LJ[6 + j] + N[6 + i] * LJ[12 + j] + T[i] * LJ[18 + j] + T[3 + i] * LJ[24 + j] + T[6 + i] * LJ[30 + j];
            else h = G[i - 3] * LJ[18 + j] + G[i] * LJ[24 + j] + G[3 + i] * LJ[30 + j];
            rec[k++] = h;
        }
    }
#pragma unroll
    for (int i = 0; i < 6; i++) {
        double g;
        if (i < 3) g = N[i] * Le[0] + N[3 + i] * Le[1] + N[6 + i] * Le[2] + T[i] * Le[3] + T[3 + i] * Le[4] + T[6 + i] * Le[5];
        else g = G[i - 3] * Le[3] + G[i] * Le[4] + G[3 + i] * Le[5];
        rec[21 + i] = g;
    }
}

template <bool LDS>
__global__ void __launch_bounds__(PAIR_THREADS) k_pair_prior(const PairPriorArgs a) {
    constexpr int NP = LDS ? PAIR_LDS_MAX : 1;
    __shared__ double s_rec[NP * PAIR_REC], s_cost[NP];
    __shared__ int32_t s_el_ent[2 * NP], s_el_start[2 * NP + 1], s_el_item[2 * NP];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (LDS) {   // the lists: read while phase 1 computes, used behind the barrier
        for (int i = tid; i < a.n_el; i += PAIR_THREADS) s_el_ent[i] = a.el_ent[i];
        for (int i = tid; i <= a.n_el; i += PAIR_THREADS) s_el_start[i] = a.el_start[i];
        for (int i = tid; i < a.n_items; i += PAIR_THREADS) s_el_item[i] = a.el_item[i];
    }
    const int32_t *el_ent = LDS ? s_el_ent : a.el_ent, *el_start = LDS ? s_el_start : a.el_start, *el_item = LDS ? s_el_item : a.el_item;
    const double *recs = LDS ? s_rec : a.rec;
    for (int p = tid; p < a.n; p += PAIR_THREADS) {
        const int ea = a.ends[4 * p], eb = a.ends[4 * p + 1], both = a.ends[4 * p + 2];
        const double *dat = a.dat + (size_t)p * PRIOR_DAT;
        double e[6], Na[9], Ta[9], Nb[9], G[9];   // J_a = [Na 0; Ta -G], J_b = [Nb 0; 0 G], G = R_a^T
        {
            Ent A, B;
            load_ent(a.ent, ea, A);
            load_ent(a.ent, eb, B);
            double rr[ENT_STRIDE];
            make_ent_row(dat, rr);   // R_rel by the Rodrigues formula of every other entity row
            double Rab[9], Q[9];
#pragma unroll
            for (int i = 0; i < 3; i++)
#pragma unroll
                for (int j = 0; j < 3; j++) {
                    G[3 * i + j] = A.R[3 * j + i];
                    Rab[3 * i + j] = A.R[i] * B.R[j] + A.R[3 + i] * B.R[3 + j] + A.R[6 + i] * B.R[6 + j];
                }
#pragma unroll
            for (int i = 0; i < 3; i++)
#pragma unroll
                for (int j = 0; j < 3; j++) Q[3 * i + j] = rr[i] * Rab[j] + rr[3 + i] * Rab[3 + j] + rr[6 + i] * Rab[6 + j];
            double phi[3], th, Ji[9], JR[9];
            so3_log(Q, phi, th);
            so3_jr_inv(phi, th, Ji);
            // JR = J_r(phi)^-1 R_b^T
#pragma unroll
            for (int i = 0; i < 3; i++)
#pragma unroll
                for (int j = 0; j < 3; j++) JR[3 * i + j] = Ji[3 * i] * B.R[3 * j] + Ji[3 * i + 1] * B.R[3 * j + 1] + Ji[3 * i + 2] * B.R[3 * j + 2];
            const double d0 = B.t[0] - A.t[0], d1 = B.t[1] - A.t[1], d2 = B.t[2] - A.t[2];
            // X = [d]x J_l(w_a)
            double X[9];
#pragma unroll
            for (int j = 0; j < 3; j++) {
                X[j] = d1 * A.Jl[6 + j] - d2 * A.Jl[3 + j];
                X[3 + j] = d2 * A.Jl[j] - d0 * A.Jl[6 + j];
                X[6 + j] = d0 * A.Jl[3 + j] - d1 * A.Jl[j];
            }
#pragma unroll
            for (int i = 0; i < 3; i++)
#pragma unroll
                for (int j = 0; j < 3; j++) {
                    Na[3 * i + j] = -(JR[3 * i] * A.Jl[j] + JR[3 * i + 1] * A.Jl[3 + j] + JR[3 * i + 2] * A.Jl[6 + j]);
                    Nb[3 * i + j] = JR[3 * i] * B.Jl[j] + JR[3 * i + 1] * B.Jl[3 + j] + JR[3 * i + 2] * B.Jl[6 + j];
                    Ta[3 * i + j] = G[3 * i] * X[j] + G[3 * i + 1] * X[3 + j] + G[3 * i + 2] * X[6 + j];
                }
            e[0] = phi[0]; e[1] = phi[1]; e[2] = phi[2];
#pragma unroll
            for (int i = 0; i < 3; i++) e[3 + i] = G[3 * i] * d0 + G[3 * i + 1] * d1 + G[3 * i + 2] * d2 - dat[3 + i];
        }
        double Lam[36], Le[6];
#pragma unroll
        for (int i = 0; i < 36; i++) Lam[i] = dat[6 + i];
        double cost = 0.0;
#pragma unroll
        for (int r = 0; r < 6; r++) {
            double s = 0.0;
#pragma unroll
            for (int c = 0; c < 6; c++) s += Lam[6 * r + c] * e[c];
            Le[r] = s;
        }
#pragma unroll
        for (int r = 0; r < 6; r++) cost += e[r] * Le[r];
        if (a.add) {
            double *rec = (LDS ? s_rec : a.rec) + (size_t)p * PAIR_REC;
            double nG[9];
#pragma unroll
            for (int i = 0; i < 9; i++) nG[i] = -G[i];
            // L J_a (row-major 6 x 6), side a's record
            double LJ[36];
#pragma unroll
            for (int r = 0; r < 6; r++)
#pragma unroll
                for (int j = 0; j < 3; j++) {
                    LJ[6 * r + j] = Lam[6 * r] * Na[j] + Lam[6 * r + 1] * Na[3 + j] + Lam[6 * r + 2] * Na[6 + j] + Lam[6 * r + 3] * Ta[j] + Lam[6 * r + 4] * Ta[3 + j] +
                                    Lam[6 * r + 5] * Ta[6 + j];
                    LJ[6 * r + 3 + j] = Lam[6 * r + 3] * nG[j] + Lam[6 * r + 4] * nG[3 + j] + Lam[6 * r + 5] * nG[6 + j];
                }
            side_record(Na, Ta, nG, LJ, Le, rec);
            if (both) {
                // X = J_b^T (L J_a): block (b, a) of the matrix; the stored lower triangle holds it as it is for b > a and transposed for a > b
                const int hi = ea > eb ? ea : eb, lo = ea > eb ? eb : ea;
                double *S = a.S + (size_t)(6 * hi) * a.n_pad + 6 * lo;
                const size_t si = ea > eb ? 1 : (size_t)a.n_pad, sj = ea > eb ? (size_t)a.n_pad : 1;
#pragma unroll
                for (int i = 0; i < 6; i++)
#pragma unroll
                    for (int j = 0; j < 6; j++) {
                        const double h = i < 3 ? Nb[i] * LJ[j] + Nb[3 + i] * LJ[6 + j] + Nb[6 + i] * LJ[12 + j]
                                               : G[i - 3] * LJ[18 + j] + G[i] * LJ[24 + j] + G[3 + i] * LJ[30 + j];
                        S[i * si + j * sj] += h;
                    }
            }
            // L J_b, side b's record
#pragma unroll
            for (int r = 0; r < 6; r++)
#pragma unroll
                for (int j = 0; j < 3; j++) {
                    LJ[6 * r + j] = Lam[6 * r] * Nb[j] + Lam[6 * r + 1] * Nb[3 + j] + Lam[6 * r + 2] * Nb[6 + j];
                    LJ[6 * r + 3 + j] = Lam[6 * r + 3] * G[j] + Lam[6 * r + 4] * G[3 + j] + Lam[6 * r + 5] * G[6 + j];
                }
            double Z[9];
#pragma unroll
            for (int i = 0; i < 9; i++) Z[i] = 0.0;
            side_record(Nb, Z, G, LJ, Le, rec + PAIR_SIDE);
        }
        double *o = a.out + (size_t)p * 8;
#pragma unroll
        for (int i = 0; i < 6; i++) o[i] = e[i];
        o[6] = cost;
        o[7] = 0.0;
        if (LDS) s_cost[p] = cost;
    }
    __syncthreads();
    if (a.add) {
        // one writer per value: 32 threads an entity (27 at work), its pairs in ascending order
        const int v = tid & 31;
        if (v < PAIR_SIDE) {
            // value v of a side's record -> its place in S (lower triangle of the diagonal block) or g0
            int row = 0;
            while (row < 5 && (row + 1) * (row + 2) / 2 <= v) row++;
            const int col = v - row * (row + 1) / 2;
            constexpr int EPR = PAIR_THREADS / 32;   // entities a round
            for (int k0 = tid >> 5; k0 < a.n_el; k0 += 4 * EPR) {
                double *dst[4];
                double old[4], s[4];
#pragma unroll
                for (int r = 0; r < 4; r++) {
                    const int k = k0 + r * EPR;
                    const int ent = k < a.n_el ? el_ent[k] : -1;
                    dst[r] = ent < 0 ? nullptr : (v < 21 ? a.S + (size_t)(6 * ent + row) * a.n_pad + 6 * ent + col : a.g0 + 6 * ent + (v - 21));
                }
#pragma unroll
                for (int r = 0; r < 4; r++) old[r] = dst[r] ? *dst[r] : 0.0;
#pragma unroll
                for (int r = 0; r < 4; r++) {
                    const int k = k0 + r * EPR;
                    s[r] = 0.0;
                    if (dst[r])
                        for (int q = el_start[k]; q < el_start[k + 1]; q++) {
                            const int it = el_item[q];
                            s[r] += recs[(size_t)(it >> 1) * PAIR_REC + (it & 1) * PAIR_SIDE + v];
                        }
                }
#pragma unroll
                for (int r = 0; r < 4; r++)
                    if (dst[r]) *dst[r] = v < 21 ? old[r] + s[r] : old[r] - s[r];
            }
        }
    }
    if (wave != 0) return;
    // the summed cost in a fixed order: lane l adds pairs l, l + 64, ... ascending, then a fixed xor tree
    double s = 0.0;
    for (int p = lane; p < a.n; p += 64) s += LDS ? s_cost[p] : a.out[(size_t)p * 8 + 6];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off);
    if (lane == 0) {
        a.out[(size_t)a.n * 8] = s;
        if (a.add) *a.err_slot = a.err_acc ? *a.err_slot + s : s;
    }
}

}  // namespace

void launch_pair_prior(const DeviceProblem &P, int which, bool add, hipStream_t st) {
    if (P.n_pair == 0) return;
    PairPriorArgs a;
    a.ends = P.pair_ends; a.dat = P.pair_dat; a.ent = P.ent[which];
    a.el_ent = P.pair_el_ent; a.el_start = P.pair_el_start; a.el_item = P.pair_el_item;
    a.n = P.n_pair; a.n_el = P.n_pair_el; a.n_items = P.n_pair_items; a.n_pad = P.n_pad;
    a.add = (add && P.prior_rank0) ? 1 : 0;
    a.err_acc = P.n_prior > 0 ? 1 : 0;
    a.S = P.blk[which].S; a.g0 = P.blk[which].g0; a.err_slot = P.err_part + P.F;
    a.rec = P.pair_rec_ws; a.out = P.pair_out;
    HookScope _h(P, KID_PRIOR);   // booked with k_prior: the kernel ids are part of the interface
    if (P.n_pair <= PAIR_LDS_MAX) hipLaunchKernelGGL(k_pair_prior<true>, dim3(1), dim3(PAIR_THREADS), 0, st, a);
    else hipLaunchKernelGGL(k_pair_prior<false>, dim3(1), dim3(PAIR_THREADS), 0, st, a);
}

}  // namespace aar
