// Covariance of a solved problem (aar_problem_covariance): the dense inverse of the reduced system S from its LDL^T factor,
// and the per-frame marginal blocks.  See DESIGN.md section 13.
//
//   k_cov_stage      S (stride n_pad) -> a copy with one extra padding tile (stride n_pad + CHOL_NB), rows without an unknown
//                    (mask) set to identity.  The extra tile makes the last real tile an ordinary one, whose factor the k_ldl_*
//                    chain keeps in Dfac (the chain itself does not store the factor of its last tile).
//   k_cov_gather     the factor as the chain leaves it (diagonal tiles in Dfac, block columns of L in place or in Lp) -> dense
//                    unit-lower L and 1 / D
//   k_cov_linv_diag  inverses of the 32 x 32 diagonal blocks of L
//   k_cov_linv_row   block row I of X = L^-1: X_IJ = -X_II sum_{K=J}^{I-1} L_IK X_KJ (one launch per block row, J parallel)
//   k_cov_sinv       S^-1 = X^T D^-1 X, lower 32 x 32 tiles only
//   k_cov_frames     Sigma_ff = V_f^-1 + sum_{a,b} G_a S^-1_ab G_b^T, G_a = V_f^-1 W_a^T: one wavefront per frame
// fp64 throughout.
#include "kernels.h"

namespace aar {

namespace {
constexpr int CT = 32;   // tile of the inverse kernels
}

__global__ void __launch_bounds__(256) k_cov_stage(const double *__restrict__ S, int n_pad, double *__restrict__ S2, int n2,
                                                   const int32_t *__restrict__ rowmask) {
    const int i = blockIdx.y, j = blockIdx.x * 256 + threadIdx.x;
    if (j >= n2 || i >= n2) return;
    double v = 0.0;
    if (i < n_pad && j < n_pad && j <= i) {
        if (rowmask[i] || rowmask[j]) v = (i == j) ? 1.0 : 0.0;
        else v = S[(size_t)i * n_pad + j];
    }
    S2[(size_t)i * n2 + j] = v;
}

// L and 1 / D of the factor the chain left for the staged system (n2 = its stride, nT2 its tiles, fused_m its panel rule)
__global__ void __launch_bounds__(256) k_cov_gather(const double *__restrict__ S2, const double *__restrict__ Dfac, const double *__restrict__ Lp,
                                                    int n_pad, int n2, int nT2, int fused_m, double *__restrict__ Lc, double *__restrict__ Dinv) {
    const int i = blockIdx.y, j = blockIdx.x * 256 + threadIdx.x;
    if (j >= n_pad) return;
    const int ti = i / CHOL_NB, tj = j / CHOL_NB;
    double v = 0.0;
    if (j == i) {
        v = 1.0;
        Dinv[i] = 1.0 / Dfac[(size_t)ti * CHOL_NB * CHOL_NB + (size_t)(i % CHOL_NB) * CHOL_NB + i % CHOL_NB];
    } else if (j < i) {
        if (ti == tj) v = Dfac[(size_t)ti * CHOL_NB * CHOL_NB + (size_t)(i % CHOL_NB) * CHOL_NB + j % CHOL_NB];
        else if (nT2 - tj - 1 <= fused_m) v = Lp[((size_t)tj * n2 + i) * CHOL_NB + j % CHOL_NB];   // (k_ldl_panel's block columns)
        else v = S2[(size_t)i * n2 + j];                                                            // (k_ldl_trsm's: in place)
    }
    Lc[(size_t)i * n_pad + j] = v;
}

// X_II = L_II^-1 (unit lower): thread c solves column c
__global__ void __launch_bounds__(CT) k_cov_linv_diag(const double *__restrict__ Lc, int n_pad, double *__restrict__ X) {
    __shared__ double Ls[CT][CT + 1];
    const int I = blockIdx.x, c = threadIdx.x, o = I * CT;
    for (int r = 0; r < CT; r++) Ls[r][c] = Lc[(size_t)(o + r) * n_pad + o + c];
    __syncthreads();
    double x[CT];
#pragma unroll
    for (int i = 0; i < CT; i++) {
        double a = (i == c) ? 1.0 : 0.0;
#pragma unroll
        for (int k = 0; k < i; k++) a = fma(-Ls[i][k], x[k], a);
        x[i] = (i < c) ? 0.0 : a;
    }
#pragma unroll
    for (int i = 0; i < CT; i++) X[(size_t)(o + i) * n_pad + o + c] = x[i];
}

// 32 x 32 tile product on 256 threads: thread (ty, tx) owns rows 4 ty .. 4 ty + 3 of column tx
__device__ __forceinline__ void tile_fma(const double (*A)[CT + 1], const double (*B)[CT + 1], int ty, int tx, double acc[4]) {
#pragma unroll
    for (int k = 0; k < CT; k++) {
        const double b = B[k][tx];
#pragma unroll
        for (int r = 0; r < 4; r++) acc[r] = fma(A[4 * ty + r][k], b, acc[r]);
    }
}

__global__ void __launch_bounds__(256) k_cov_linv_row(const double *__restrict__ Lc, int n_pad, int I, double *__restrict__ X) {
    __shared__ double As[CT][CT + 1], Bs[CT][CT + 1];
    const int J = blockIdx.x, tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    double acc[4] = {0.0, 0.0, 0.0, 0.0};
    for (int K = J; K < I; K++) {
        for (int e = threadIdx.x; e < CT * CT; e += 256) {
            const int r = e >> 5, c = e & 31;
            As[r][c] = Lc[(size_t)(I * CT + r) * n_pad + K * CT + c];
            Bs[r][c] = X[(size_t)(K * CT + r) * n_pad + J * CT + c];
        }
        __syncthreads();
        tile_fma(As, Bs, ty, tx, acc);
        __syncthreads();
    }
    for (int e = threadIdx.x; e < CT * CT; e += 256) {
        const int r = e >> 5, c = e & 31;
        As[r][c] = X[(size_t)(I * CT + r) * n_pad + I * CT + c];
    }
#pragma unroll
    for (int r = 0; r < 4; r++) Bs[4 * ty + r][tx] = acc[r];
    __syncthreads();
    double x[4] = {0.0, 0.0, 0.0, 0.0};
    tile_fma(As, Bs, ty, tx, x);
#pragma unroll
    for (int r = 0; r < 4; r++) X[(size_t)(I * CT + 4 * ty + r) * n_pad + J * CT + tx] = -x[r];
}

// Sinv_AB = sum_{K >= A} X_KA^T D_K^-1 X_KB for the lower tiles A >= B (blockIdx.x enumerates them row by row)
__global__ void __launch_bounds__(256) k_cov_sinv(const double *__restrict__ X, const double *__restrict__ Dinv, int n_pad, int nb,
                                                  double *__restrict__ Sinv) {
    __shared__ double As[CT][CT + 1], Bs[CT][CT + 1];
    const int t = blockIdx.x;
    int A = (int)((sqrt(8.0 * t + 1.0) - 1.0) * 0.5);
    while (A * (A + 1) / 2 > t) A--;
    while ((A + 1) * (A + 2) / 2 <= t) A++;
    const int B = t - A * (A + 1) / 2;
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    double acc[4] = {0.0, 0.0, 0.0, 0.0};
    for (int K = A; K < nb; K++) {
        for (int e = threadIdx.x; e < CT * CT; e += 256) {
            const int r = e >> 5, c = e & 31;
            const size_t row = (size_t)(K * CT + r) * n_pad;
            As[c][r] = X[row + A * CT + c] * Dinv[K * CT + r];   // transposed: As[i][k] = X[k][i] / D_k
            Bs[r][c] = X[row + B * CT + c];
        }
        __syncthreads();
        tile_fma(As, Bs, ty, tx, acc);
        __syncthreads();
    }
#pragma unroll
    for (int r = 0; r < 4; r++) Sinv[(size_t)(A * CT + 4 * ty + r) * n_pad + B * CT + tx] = acc[r];
}

// One wavefront per frame: G_s = V_f^-1 W_s^T for its slots (columns of rows without an unknown zeroed) into LDS, then the
// lanes share the slot pairs a <= b, each accumulating its 36 entries of sum G_a Sinv_ab G_b^T (a < b counted once, the
// transpose added at the end), a butterfly over the wavefront, V_f^-1 added.  A frame without observations gets NaN.
__global__ void __launch_bounds__(64) k_cov_frames(const int32_t *__restrict__ fslot_start, const int32_t *__restrict__ fslot_ent,
                                                   const double *__restrict__ W, const double *__restrict__ Vinv, const double *__restrict__ Sinv,
                                                   const int32_t *__restrict__ rowmask, int n_pad, int F, double *__restrict__ out) {
    extern __shared__ double G[];   // [max_kf][36] | entity of each slot as double
    const int f = blockIdx.x, lane = threadIdx.x;
    if (f >= F) return;
    const int s0 = fslot_start[f], ks = fslot_start[f + 1] - s0;
    if (ks == 0) {
        if (lane < 36) out[(size_t)f * 36 + lane] = __builtin_nan("");
        return;
    }
    double *ent = G + (size_t)ks * 36;
    for (int e = lane; e < ks * 36; e += 64) {
        const int s = e / 36, p = (e % 36) / 6, q = e % 6;   // G_s[p][q] = sum_r Vinv[p][r] W_s[q][r]
        const int a = fslot_ent[s0 + s];
        double v = 0.0;
        if (!rowmask[6 * a + q]) {
            const double *w = W + (size_t)(s0 + s) * 36 + q * 6, *vi = Vinv + (size_t)f * 36 + p * 6;
#pragma unroll
            for (int r = 0; r < 6; r++) v = fma(vi[r], w[r], v);
        }
        G[e] = v;
        if (e % 36 == 0) ent[s] = (double)a;
    }
    __syncthreads();
    double acc[36];
#pragma unroll
    for (int i = 0; i < 36; i++) acc[i] = 0.0;
    const int npairs = ks * (ks + 1) / 2;
    for (int t = lane; t < npairs; t += 64) {
        int b = (int)((sqrt(8.0 * t + 1.0) - 1.0) * 0.5);   // pair t = (a, b), a <= b, enumerated b-major
        while (b * (b + 1) / 2 > t) b--;
        while ((b + 1) * (b + 2) / 2 <= t) b++;
        const int a = t - b * (b + 1) / 2;
        const int ea = (int)ent[a], eb = (int)ent[b];
        const double *Ga = G + a * 36, *Gb = G + b * 36;
        double sab[36];   // Sinv rows of entity ea, columns of entity eb, read from the stored lower triangle
#pragma unroll
        for (int i = 0; i < 6; i++)
#pragma unroll
            for (int j = 0; j < 6; j++) {
                const int r = 6 * ea + i, c = 6 * eb + j;
                sab[i * 6 + j] = r >= c ? Sinv[(size_t)r * n_pad + c] : Sinv[(size_t)c * n_pad + r];
            }
        const double wgt = (a == b) ? 0.5 : 1.0;
        double tmp[36];   // Ga Sab
#pragma unroll
        for (int p = 0; p < 6; p++)
#pragma unroll
            for (int j = 0; j < 6; j++) {
                double v = 0.0;
#pragma unroll
                for (int i = 0; i < 6; i++) v = fma(Ga[p * 6 + i], sab[i * 6 + j], v);
                tmp[p * 6 + j] = v * wgt;
            }
#pragma unroll
        for (int p = 0; p < 6; p++)
#pragma unroll
            for (int q = 0; q < 6; q++) {
                double v = acc[p * 6 + q];
#pragma unroll
                for (int j = 0; j < 6; j++) v = fma(tmp[p * 6 + j], Gb[q * 6 + j], v);
                acc[p * 6 + q] = v;
            }
    }
#pragma unroll
    for (int i = 0; i < 36; i++) {
        double v = acc[i];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
        acc[i] = v;
    }
    if (lane < 36) {
        const int p = lane / 6, q = lane % 6;
        double v = 0.0;
#pragma unroll
        for (int i = 0; i < 36; i++) v = (i == lane) ? v + acc[i] : v;
#pragma unroll
        for (int i = 0; i < 36; i++) v = (i == q * 6 + p) ? v + acc[i] : v;
        out[(size_t)f * 36 + lane] = Vinv[(size_t)f * 36 + lane] + v;
    }
}

// the 6x6 diagonal blocks of every entity out of the lower triangle of Sinv: out[a][36]
__global__ void __launch_bounds__(256) k_cov_diag_blocks(const double *__restrict__ Sinv, int n_pad, int A, double *__restrict__ out) {
    const int g = blockIdx.x * 256 + threadIdx.x;
    if (g >= 36 * A) return;
    const int a = g / 36, i = (g % 36) / 6, j = g % 6, r = 6 * a + (i > j ? i : j), c = 6 * a + (i > j ? j : i);
    out[g] = Sinv[(size_t)r * n_pad + c];
}

void launch_cov_diag_blocks(const double *Sinv, int n_pad, int A, double *out, hipStream_t st) {
    if (A > 0) hipLaunchKernelGGL(k_cov_diag_blocks, dim3((unsigned)((36 * A + 255) / 256)), dim3(256), 0, st, Sinv, n_pad, A, out);
}

void launch_cov_stage(const double *S, int n_pad, double *S2, int n2, const int32_t *rowmask, hipStream_t st) {
    hipLaunchKernelGGL(k_cov_stage, dim3((unsigned)((n2 + 255) / 256), (unsigned)n2), dim3(256), 0, st, S, n_pad, S2, n2, rowmask);
}

void launch_cov_inverse(const double *S2, const double *Dfac, const double *Lp, int n_pad, int n2, int nT2, int fused_m, double *Lc, double *Dinv,
                        double *X, double *Sinv, hipStream_t st) {
    const int nb = n_pad / CT;
    hipLaunchKernelGGL(k_cov_gather, dim3((unsigned)((n_pad + 255) / 256), (unsigned)n_pad), dim3(256), 0, st, S2, Dfac, Lp, n_pad, n2, nT2, fused_m, Lc, Dinv);
    hipLaunchKernelGGL(k_cov_linv_diag, dim3((unsigned)nb), dim3(CT), 0, st, Lc, n_pad, X);
    for (int I = 1; I < nb; I++) hipLaunchKernelGGL(k_cov_linv_row, dim3((unsigned)I), dim3(256), 0, st, Lc, n_pad, I, X);
    hipLaunchKernelGGL(k_cov_sinv, dim3((unsigned)(nb * (nb + 1) / 2)), dim3(256), 0, st, X, Dinv, n_pad, nb, Sinv);
}

void launch_cov_frames(const DeviceProblem &P, int which, const double *Sinv, const int32_t *rowmask, double *out, hipStream_t st) {
    if (P.F == 0) return;
    const size_t lds = ((size_t)std::max(P.max_kf, 1) * 37) * sizeof(double);
    launch_lds(k_cov_frames, dim3((unsigned)P.F), dim3(64), lds, st, P.fslot_start, P.fslot_ent, P.blk[which].W, P.blk[which].Vinv, Sinv, rowmask,
               P.n_pad, P.F, out);
}

}  // namespace aar
