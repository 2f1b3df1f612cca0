// The per-frame evaluation of track(): one wavefront sums a frame's weighted squared residuals and, optionally, its 6x6 normal
// equations V (21 packed) and right-hand side g = -J^T r_w.  Shared by k_track (eval_kernels.hip) and the smoothed tracker
// (smooth_kernels.hip); see the track() notes in eval_kernels.hip for the model.
#pragma once
#include "geom.hpp"
#include "kernels.h"

namespace aar {

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
    return v;
}

struct TrackArgs {
    const ObsIdx *idx; const float *uv; const double *ent; const double *Kmat; const int32_t *frame_obs_start;
    int kstride;
    int A, F; float huber; double h;
    int max_iters; double min_error, min_step_error_diff, min_average_step_error_diff, tau;
    double *z;            // [6(A+F)]: frame poses in/out
    int32_t *iters_out;   // [F]
    double *err_out;      // [F]
};

// residual sum (and optionally V (21 packed), g (6)) of the observations [o0, o1) at pose zf, summed over the wave.  Observation o has its
// ObsIdx at idx + o * IDX_STRIDE bytes and its eight corner coordinates at uv + o * UV_STRIDE bytes (16-byte aligned): the problem's
// two arrays (strides 16 and 32), or the interleaved records of the live tracker's ring (live_kernels.hip).  Reads a.ent, a.Kmat, a.kstride,
// a.huber, a.h.
template <bool WITH_J, int IDX_STRIDE, int UV_STRIDE>
__device__ __forceinline__ double track_eval_range(const TrackArgs &a, const char *idx, const char *uv, int o0, int o1, const double zf[6], int lane,
                                                   double V[21], double g[6]) {
    double row[ENT_STRIDE];
    make_ent_row(zf, row);
    Ent ef;
#pragma unroll
    for (int i = 0; i < 9; i++) { ef.R[i] = row[i]; ef.Jl[i] = row[12 + i]; }
#pragma unroll
    for (int i = 0; i < 3; i++) ef.t[i] = row[9 + i];
    double acc[28];
#pragma unroll
    for (int i = 0; i < 28; i++) acc[i] = 0.0;
    for (int o = o0 + lane; o < o1; o += 64) {
        const ObsIdx id = *reinterpret_cast<const ObsIdx *>(idx + (int64_t)o * IDX_STRIDE);
        const float4 uv0 = reinterpret_cast<const float4 *>(uv + (int64_t)o * UV_STRIDE)[0];
        const float4 uv1 = reinterpret_cast<const float4 *>(uv + (int64_t)o * UV_STRIDE)[1];
        const float ou[8] = {uv0.x, uv0.y, uv0.z, uv0.w, uv1.x, uv1.y, uv1.z, uv1.w};
        Ent ec, em;
        load_ent(a.ent, id.cam, ec);
        load_ent(a.ent, id.marker, em);
        double K[9];
#pragma unroll
        for (int i = 0; i < 9; i++) K[i] = a.Kmat[a.kstride * id.cam + i];
#pragma unroll
        for (int k = 0; k < 4; k++) {
            CornerGeom gm;
            project_corner(ec, em, ef, K, a.h, k, gm);
            double r[2];
            corner_residual(ou[2 * k], ou[2 * k + 1], gm.u, gm.v, 0, -1.f, r[0], r[1]);  // double residuals (:712-713), unweighted
            // Huber: track() differentiates the WEIGHTED error function numerically (calcDerivates), so the weight's own
            // derivative belongs to the Jacobian here (unlike solve(), whose Jacobian ignores the weights):
            //   r_w = w r,  w = sqrt(rho)/s,  s = |r|,  rho = 2 delta s - delta^2  (outliers; w = 1 otherwise)
            //   d r_w = w dr + r (dw/ds) (r . dr)/s
            double w = 1.0, cw = 0.0;
            if (a.huber >= 0.f) {
                const double e = r[0] * r[0] + r[1] * r[1];
                const float dsq = a.huber * a.huber, d2 = 2 * a.huber;
                if (e != 0.0 && e > (double)dsq) {
                    const double sn = sqrt(e), rho = (double)d2 * sn - (double)dsq, sr = sqrt(rho);
                    w = sr / sn;
                    cw = ((double)a.huber / sr - sr / sn) / e;  // (dw/ds) / s
                }
            }
            acc[27] += w * w * (r[0] * r[0] + r[1] * r[1]);
            if (WITH_J) {
                double Gc[2][6], Gm[2][6], Gf[2][6];
                corner_jacobian<false, false, true>(ec, em, ef, K, gm, Gc, Gm, Gf);
                if (cw != 0.0 || w != 1.0) {
#pragma unroll
                    for (int i = 0; i < 6; i++) {
                        const double rg = r[0] * Gf[0][i] + r[1] * Gf[1][i];
                        Gf[0][i] = w * Gf[0][i] + cw * r[0] * rg;
                        Gf[1][i] = w * Gf[1][i] + cw * r[1] * rg;
                    }
                }
                r[0] *= w;
                r[1] *= w;
#pragma unroll
                for (int rr = 0; rr < 2; rr++)
#pragma unroll
                    for (int i = 0; i < 6; i++) {
                        acc[21 + i] += Gf[rr][i] * r[rr];
#pragma unroll
                        for (int j = 0; j <= i; j++) acc[i * (i + 1) / 2 + j] += Gf[rr][i] * Gf[rr][j];
                    }
            }
        }
    }
    if (WITH_J) {
#pragma unroll
        for (int i = 0; i < 21; i++) V[i] = wave_sum(acc[i]);
#pragma unroll
        for (int i = 0; i < 6; i++) g[i] = wave_sum(acc[21 + i]);
    }
    return wave_sum(acc[27]);
}

// ... of frame f of the problem behind a
template <bool WITH_J>
__device__ __forceinline__ double track_eval(const TrackArgs &a, int f, const double zf[6], int lane, double V[21], double g[6]) {
    return track_eval_range<WITH_J, (int)sizeof(ObsIdx), 32>(a, reinterpret_cast<const char *>(a.idx), reinterpret_cast<const char *>(a.uv),
                                                             a.frame_obs_start[f], a.frame_obs_start[f + 1], zf, lane, V, g);
}

}  // namespace aar
