// Fitting the smoother's noise levels: the expected sufficient statistics of the between factors under the Laplace
// posterior N(z, q H^-1), from the diagonal and lag-one blocks S[f] = (H^-1)_ff, R[f] = (H^-1)_{f,f+1} that launch_smooth_selinv left on
// the device.  Per pair f (g = f + 1, D = frame_time[g] - frame_time[f]), with phi, e_t, M_a, M_b of pair_terms<true> at z:
//   a_r = |phi|^2 / D     u_r = tr(M_a S_ff^ww M_a^T + M_b S_gg^ww M_b^T + M_a R_f^ww M_b^T + M_b R_f^ww^T M_a^T) / D
//   a_t = |e_t|^2 / D     u_t = tr(S_ff^tt + S_gg^tt - R_f^tt - R_f^tt^T) / D
// (the linearised e_f moves by J_a dz_f + J_b dz_g, J_a = [M_a 0; 0 -I], J_b = [M_b 0; 0 I]; ^ww / ^tt: the rotation / translation 3x3
// sub-blocks).  The host holds sigma^2 D, not D: 1 / D = lam_r sigma_rot^2 is passed as lam and the sigma's square.
//   k_smooth_fit_terms    one thread per pair -> terms [F-1][4] = a_r, u_r, a_t, u_t
//   k_smooth_fit_reduce   one workgroup: thread t adds entries t, t + 256, ... ascending, then a fixed tree -> rec[0..3] the four sums,
//                         rec[4], rec[5] the data and prior cost of the evaluation's record, rec[6] the elimination's pivot flag
// No atomics, one owner per store, a fixed order: the same bits from call to call.
#include "geom.hpp"
#include "kernels.h"
#include "pair_terms.hpp"
#include "so3.hpp"

namespace aar {

namespace {

__global__ void __launch_bounds__(64) k_smooth_fit_terms(const double *z, const double *rel, const double *lam, double sr2, const double *S,
                                                         const double *R, int F, double *terms) {
    const int f = blockIdx.x * 64 + threadIdx.x;
    if (f + 1 >= F) return;
    double za[6], zb[6], ra[ENT_STRIDE], rb[ENT_STRIDE];
    ld6(z + 6 * (size_t)f, za);
    ld6(z + 6 * (size_t)f + 6, zb);
    make_ent_row(za, ra);
    make_ent_row(zb, rb);
    double phi[3], et[3], Ma[9], Mb[9];
    pair_terms<true>(ra, rb, rel ? rel + 6 * (size_t)f : nullptr, phi, et, Ma, Mb);
    const double inv_dt = lam[2 * (size_t)f] * sr2;   // lam_r = 1 / (sigma_rot^2 D)
    const double *sf = S + 36 * (size_t)f, *sg = sf + 36, *rf = R + 36 * (size_t)f;
    // u_r = sum_ij (M_a S_ff^ww)_ij M_a_ij + (M_b S_gg^ww)_ij M_b_ij + 2 (M_a R^ww)_ij M_b_ij
    double ur = 0.0, ut = 0.0;
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int j = 0; j < 3; j++) {
            double x = 0.0, y = 0.0, w = 0.0;
#pragma unroll
            for (int k = 0; k < 3; k++) {
                x = fma(Ma[3 * i + k], sf[6 * k + j], x);
                y = fma(Mb[3 * i + k], sg[6 * k + j], y);
                w = fma(Ma[3 * i + k], rf[6 * k + j], w);
            }
            ur = fma(x, Ma[3 * i + j], ur);
            ur = fma(y, Mb[3 * i + j], ur);
            ur = fma(2.0 * w, Mb[3 * i + j], ur);
        }
#pragma unroll
    for (int i = 0; i < 3; i++) ut += sf[21 + 7 * i] + sg[21 + 7 * i] - 2.0 * rf[21 + 7 * i];
    double *o = terms + 4 * (size_t)f;
    o[0] = (phi[0] * phi[0] + phi[1] * phi[1] + phi[2] * phi[2]) * inv_dt;
    o[1] = ur * inv_dt;
    o[2] = (et[0] * et[0] + et[1] * et[1] + et[2] * et[2]) * inv_dt;
    o[3] = ut * inv_dt;
}

__global__ void __launch_bounds__(256) k_smooth_fit_reduce(const double *terms, int n, const double *res, const int32_t *flag, double *rec) {
    __shared__ double sh[4][256];
    const int t = threadIdx.x;
    double s[4] = {0.0, 0.0, 0.0, 0.0};
    for (int f = t; f < n; f += 256) {
#pragma unroll
        for (int q = 0; q < 4; q++) s[q] += terms[4 * (size_t)f + q];
    }
#pragma unroll
    for (int q = 0; q < 4; q++) sh[q][t] = s[q];
    __syncthreads();
    for (int off = 128; off > 0; off >>= 1) {
        if (t < off) {
#pragma unroll
            for (int q = 0; q < 4; q++) sh[q][t] += sh[q][t + off];
        }
        __syncthreads();
    }
    if (t < 4) rec[t] = sh[t][0];
    if (t == 4) rec[4] = res[0];
    if (t == 5) rec[5] = res[1];
    if (t == 6) rec[6] = (double)flag[0];
    if (t == 7) rec[7] = 0.0;
}

}  // namespace

// after launch_smooth_eval(.., cur, true, ..), launch_smooth_solve(w, F, 0.0, st) and launch_smooth_selinv(w, F, S, R, st) on the same stream
// (F >= 2): terms [F-1][4] and rec [8] as above; sigma_rot is the one w.lam was built with.  Two launches.
int launch_smooth_fit_terms(const SmoothWork &w, int cur, int F, double sigma_rot, const double *S, const double *R, double *terms, double *rec,
                            hipStream_t st) {
    hipLaunchKernelGGL(k_smooth_fit_terms, dim3((F - 1 + 63) / 64), dim3(64), 0, st, (const double *)w.z[cur], w.rel, (const double *)w.lam,
                       sigma_rot * sigma_rot, S, R, F, terms);
    hipLaunchKernelGGL(k_smooth_fit_reduce, dim3(1), dim3(256), 0, st, (const double *)terms, F - 1, (const double *)w.res, (const int32_t *)w.flag, rec);
    return 2;
}

}  // namespace aar
