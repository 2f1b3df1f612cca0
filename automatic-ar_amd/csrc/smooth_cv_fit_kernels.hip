// Fitting the noise levels of the constant-velocity smoother: the expected sufficient statistics of the second-difference
// terms under the Laplace posterior N(z, q H^-1), from the diagonal, lag-one and lag-two blocks fc[f] = (H^-1)_ff, lc[f] = (H^-1)_{f,f+1},
// l2[f] = (H^-1)_{f,f+2} that launch_smooth_cv_selinv left on the device.  Term f (1 <= f <= F-2, D = frame_time[f+1] - frame_time[f],
// r = ratio[f]) over the frames p = f-1, c = f, n = f+1, with phi, e_t, M_p, M_c, M_n of cv_term<true> at z and c = (r, -(1 + r), 1):
//   a_r = |phi|^2 / D     u_r = sum_{x,y in {p,c,n}} tr(M_x S_xy^ww M_y^T) / D
//   a_t = |e_t|^2 / D     u_t = sum_{x,y} c_x c_y tr(S_xy^tt) / D
// S_pp, S_cc, S_nn = fc[f-1], fc[f], fc[f+1]; S_pc, S_cn = lc[f-1], lc[f]; S_pn = l2[f-1]; the transposes supply the other three (^ww / ^tt:
// the rotation / translation 3x3 sub-blocks).  Entry 0 is pair 0 in the form of smooth_fit_kernels.hip: pair_terms<true> over the frames 0, 1
// with c = (-1, 1).  The host holds sigma^2 D, not D: 1 / D = lam_r sigma^2 with the sigma that entry's lam was built with.
//   k_smooth_cv_fit_terms    one thread per entry -> terms [F-1][4] = a_r, u_r, a_t, u_t
//   k_smooth_cv_fit_reduce   one workgroup: thread t adds the entries 1 + t, 1 + t + 256, ... ascending, then a fixed tree -> rec[0..3] the four
//                            sums over the terms 1 .. F-2, rec[4], rec[5] the data and prior cost of the evaluation's record, rec[6] the
//                            elimination's pivot flag, rec[7] = u_0 = u_r[0] / sigma_rot0^2 + u_t[0] / sigma_trans0^2, pair 0's share of the trace
// No atomics, one owner per store, a fixed order: the same bits from call to call.
#include "cv_term.hpp"
#include "geom.hpp"
#include "kernels.h"
#include "pair_terms.hpp"
#include "so3.hpp"

namespace aar {

namespace {

// sum_ij (X S^ww)_ij Y_ij = tr(X S^ww Y^T) of the 6x6 block s, read here
__device__ __forceinline__ double tr_ww(const double *X, const double *s, const double *Y) {
    double u = 0.0;
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int j = 0; j < 3; j++) {
            double x = 0.0;
#pragma unroll
            for (int k = 0; k < 3; k++) x = fma(X[3 * i + k], s[6 * k + j], x);
            u = fma(x, Y[3 * i + j], u);
        }
    return u;
}
__device__ __forceinline__ double tr_tt(const double *s) { return s[21] + s[28] + s[35]; }

__global__ void __launch_bounds__(64) k_smooth_cv_fit_terms(const double *z, const double *lam, const double *ratio, double sr2, double sr02,
                                                            const double *fc, const double *lc, const double *l2, int F, double *terms) {
    const int f = blockIdx.x * 64 + threadIdx.x;
    if (f + 1 >= F) return;
    double phi[3], et[3], Mp[9], Mc[9], Mn[9], r = 0.0;
    {
        double zc[6], zn[6], rc[ENT_STRIDE], rn[ENT_STRIDE];
        ld6(z + 6 * (size_t)f, zc);
        ld6(z + 6 * (size_t)f + 6, zn);
        make_ent_row(zc, rc);
        make_ent_row(zn, rn);
        if (f == 0) {
            pair_terms<true>(rc, rn, nullptr, phi, et, Mc, Mn);
#pragma unroll
            for (int i = 0; i < 9; i++) Mp[i] = 0.0;
        } else {
            double zp[6], rp[ENT_STRIDE];
            ld6(z + 6 * (size_t)f - 6, zp);
            make_ent_row(zp, rp);
            r = ratio[f];
            cv_term<true>(rp, rc, rn, r, phi, et, Mp, Mc, Mn);
        }
    }
    const double inv_dt = lam[2 * (size_t)f] * (f == 0 ? sr02 : sr2);   // lam_r = 1 / (sigma^2 D)
    const double cc = f == 0 ? -1.0 : -(1.0 + r);
    // the blocks of frames f, f + 1 (both kinds of entry), each streamed at its use
    const double *scc = fc + 36 * (size_t)f, *snn = scc + 36, *scn = lc + 36 * (size_t)f;
    double ur = tr_ww(Mc, scc, Mc);
    double ut = cc * cc * tr_tt(scc);
    ur += tr_ww(Mn, snn, Mn);
    ut += tr_tt(snn);
    ur = fma(2.0, tr_ww(Mc, scn, Mn), ur);
    ut = fma(2.0 * cc, tr_tt(scn), ut);
    if (f > 0) {
        // ... and those frame f - 1 takes part in
        const double *spp = scc - 36, *spc = scn - 36, *spn = l2 + 36 * (size_t)f - 36;
        ur += tr_ww(Mp, spp, Mp);
        ut = fma(r * r, tr_tt(spp), ut);
        ur = fma(2.0, tr_ww(Mp, spc, Mc), ur);
        ut = fma(2.0 * r * cc, tr_tt(spc), ut);
        ur = fma(2.0, tr_ww(Mp, spn, Mn), ur);
        ut = fma(2.0 * r, tr_tt(spn), ut);
    }
    double *o = terms + 4 * (size_t)f;
    o[0] = (phi[0] * phi[0] + phi[1] * phi[1] + phi[2] * phi[2]) * inv_dt;
    o[1] = ur * inv_dt;
    o[2] = (et[0] * et[0] + et[1] * et[1] + et[2] * et[2]) * inv_dt;
    o[3] = ut * inv_dt;
}

// n = F - 1 entries, entry 0 (pair 0) outside the sums; isr02, ist02 = 1 / sigma_rot0^2, 1 / sigma_trans0^2
__global__ void __launch_bounds__(256) k_smooth_cv_fit_reduce(const double *terms, int n, const double *res, const int32_t *flag, double isr02,
                                                              double ist02, double *rec) {
    __shared__ double sh[4][256];
    const int t = threadIdx.x;
    double s[4] = {0.0, 0.0, 0.0, 0.0};
    for (int f = 1 + t; f < n; f += 256) {
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
    if (t == 7) rec[7] = terms[1] * isr02 + terms[3] * ist02;
}

}  // namespace

// after launch_smooth_cv_eval(.., cur, true, ..), launch_smooth_cv_solve(w, F, 0.0, st) and launch_smooth_cv_selinv(w, F, .., &fc, &lc, &l2, st)
// on the same stream (F >= 3): terms [F-1][4] and rec [8] as above; sigma_rot and sigma_rot0, sigma_trans0 are the ones w.lam was built with.
// Two launches.
int launch_smooth_cv_fit_terms(const SmoothCvWork &w, int cur, int F, double sigma_rot, double sigma_rot0, double sigma_trans0, const double *fc,
                               const double *lc, const double *l2, double *terms, double *rec, hipStream_t st) {
    hipLaunchKernelGGL(k_smooth_cv_fit_terms, dim3((F - 1 + 63) / 64), dim3(64), 0, st, (const double *)w.z[cur], (const double *)w.lam,
                       (const double *)w.ratio, sigma_rot * sigma_rot, sigma_rot0 * sigma_rot0, fc, lc, l2, F, terms);
    hipLaunchKernelGGL(k_smooth_cv_fit_reduce, dim3(1), dim3(256), 0, st, (const double *)terms, F - 1, (const double *)w.res,
                       (const int32_t *)w.flag, 1.0 / (sigma_rot0 * sigma_rot0), 1.0 / (sigma_trans0 * sigma_trans0), rec);
    return 2;
}

}  // namespace aar
