// Residual report of a problem (aar_problem_residual_report): per-detection reprojection errors, their exact lower median by a radix
// select on the device, the keep flags of an outlier rule and per-camera / marker / frame statistics.  See DESIGN.md section 14.
//
//   k_rr_errors    ordering A, one wavefront per frame: e_d = sqrt(sum of the 8 squared corner residuals / 4) (unweighted, the
//                  projection of k_residual), the frame's {detections, sum r^2, max e_d}, and the histogram of the select's first digit
//   k_rr_hist      one select pass: the histogram of the next digit over the keys that carry the prefix picked so far (LDS per
//                  workgroup, merged into one global histogram); once the bucket holds a single key, that key itself
//   k_rr_pick      one workgroup: the digit whose bucket holds the wanted rank, the new prefix and remaining rank
//   k_rr_tod       (with a communicator) the histogram as doubles, the payload of the all-reduce
//   k_rr_keep      ordering A, one wavefront per frame: the threshold from the median and the rule, keep flags, rejected per frame
//   k_rr_runs      one wavefront per (camera, marker) run of ordering B (through the B -> A permutation): its sums, in a fixed order
//   k_rr_entities  one thread per camera / marker: its runs added up in ascending order
// Keys: the bits of a non-negative double are ordered as its value; NaN maps above +inf.  Every sum is taken in a fixed order
// (wave sums by xor shuffles, runs ascending), and the histograms are integer counts: two calls give the same bits.
#include "geom.hpp"
#include "kernels.h"

namespace aar {

namespace {
constexpr unsigned long long NAN_KEY = 0x7FF8000000000000ull;

__device__ __forceinline__ unsigned long long err_key(double e) {
    return isnan(e) ? NAN_KEY : ((unsigned long long)__double_as_longlong(e) & 0x7FFFFFFFFFFFFFFFull);
}
__device__ __forceinline__ double key_err(unsigned long long k) { return __longlong_as_double((long long)k); }

__device__ __forceinline__ double wave_sum_x(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ __forceinline__ int wave_sum_i(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ __forceinline__ unsigned long long wave_max_k(unsigned long long v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned long long w = (unsigned long long)__shfl_xor((long long)v, o, 64);
        v = w > v ? w : v;
    }
    return v;
}

// the digit below prefix bits [pshift, 63): its shift and width (11 bits, the last one 8: 63 = 5 * 11 + 8)
__device__ __forceinline__ int digit_shift(int pshift) { return pshift > RR_DIGIT_BITS ? pshift - RR_DIGIT_BITS : 0; }

// LDS histogram -> global: only the bins that were hit
__device__ __forceinline__ void merge_hist(const uint32_t *lh, uint32_t *__restrict__ hist, int nb) {
    for (int b = threadIdx.x; b < nb; b += blockDim.x) {
        const uint32_t c = lh[b];
        if (c) atomicAdd(&hist[b], c);
    }
}
}  // namespace

// ------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) k_rr_errors(const ObsIdx *__restrict__ idx, const float *__restrict__ uv, const double *__restrict__ ent,
                                                   const double *__restrict__ Kmat, int kstride, const int32_t *__restrict__ frame_obs_start,
                                                   int F, int A, double h, int res_f32, double *__restrict__ err, double *__restrict__ ss_out,
                                                   double *__restrict__ fstat, uint32_t *__restrict__ hist, RRSel *__restrict__ sel,
                                                   unsigned long long rank) {
    __shared__ uint32_t lh[RR_BINS];
    for (int b = threadIdx.x; b < RR_BINS; b += blockDim.x) lh[b] = 0;
    if (blockIdx.x == 0 && threadIdx.x == 0) {   // the select starts here: every key carries the empty prefix
        RRSel s;
        s.prefix = 0; s.rank = rank; s.t = 0.0; s.pshift = 63; s.done = 0; s.single = 0; s.pad = 0;
        *sel = s;
    }
    __syncthreads();
    const int lane = threadIdx.x & 63, f = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (f < F) {
        const int o0 = frame_obs_start[f], o1 = frame_obs_start[f + 1];
        double fss = 0.0;
        unsigned long long mk = 0;
        for (int o = o0 + lane; o < o1; o += 64) {
            const ObsIdx id = idx[o];
            const float4 uv0 = reinterpret_cast<const float4 *>(uv)[2 * (size_t)o];
            const float4 uv1 = reinterpret_cast<const float4 *>(uv)[2 * (size_t)o + 1];
            const float ou[8] = {uv0.x, uv0.y, uv0.z, uv0.w, uv1.x, uv1.y, uv1.z, uv1.w};
            EntRT ec, em, ef;
            load_ent_rt(ent, id.cam, ec);
            load_ent_rt(ent, id.marker, em);
            load_ent_rt(ent, A + id.frame, ef);
            double K[9];
#pragma unroll
            for (int i = 0; i < 9; i++) K[i] = Kmat[kstride * id.cam + i];
            double ss = 0.0;
#pragma unroll
            for (int k = 0; k < 4; k++) {
                CornerGeom g;
                project_corner(ec, em, ef, K, h, k, g);
                double rx, ry;
                corner_residual(ou[2 * k], ou[2 * k + 1], g.u, g.v, res_f32, -1.f, rx, ry);   // unweighted, whatever the problem's Huber setting
                ss += rx * rx + ry * ry;
            }
            const double e = sqrt(ss / 4.0);
            err[o] = e;
            ss_out[o] = ss;
            fss += ss;
            const unsigned long long key = err_key(e);
            mk = key > mk ? key : mk;
            atomicAdd(&lh[(unsigned)(key >> (63 - RR_DIGIT_BITS))], 1u);
        }
        fss = wave_sum_x(fss);
        mk = wave_max_k(mk);
        if (lane == 0) {
            fstat[4 * (size_t)f + 0] = (double)(o1 - o0);
            fstat[4 * (size_t)f + 1] = fss;
            fstat[4 * (size_t)f + 2] = key_err(mk);
            fstat[4 * (size_t)f + 3] = 0.0;
        }
    }
    __syncthreads();
    merge_hist(lh, hist, RR_BINS);
}

// ------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) k_rr_hist(const double *__restrict__ err, int64_t N, uint32_t *__restrict__ hist, const RRSel *__restrict__ sel) {
    __shared__ uint32_t lh[RR_BINS];
    const RRSel s = *sel;
    if (s.done) return;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    const unsigned long long want = s.prefix >> s.pshift;
    if (s.single) {   // one key carries the prefix (on one rank): it is the answer
        for (int64_t o = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; o < N; o += stride) {
            const unsigned long long key = err_key(err[o]);
            if ((key >> s.pshift) == want) { hist[RR_BINS] = (uint32_t)(key >> 32); hist[RR_BINS + 1] = (uint32_t)key; }
        }
        return;
    }
    const int sh = digit_shift(s.pshift);
    const unsigned mask = (1u << (s.pshift - sh)) - 1u;
    for (int b = threadIdx.x; b < RR_BINS; b += blockDim.x) lh[b] = 0;
    __syncthreads();
    for (int64_t o = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; o < N; o += stride) {
        const unsigned long long key = err_key(err[o]);
        if ((key >> s.pshift) == want) atomicAdd(&lh[(unsigned)(key >> sh) & mask], 1u);
    }
    __syncthreads();
    merge_hist(lh, hist, (int)mask + 1);
}

// ------------------------------------------------------------------------------------------------
// one workgroup of 256: thread t owns bins [8t, 8t + 8).  Counts are read as doubles (exact below 2^53): from the all-reduced copy
// hd when there is one, else from hist.  Clears hist for the next pass.
__global__ void __launch_bounds__(256) k_rr_pick(uint32_t *__restrict__ hist, const double *__restrict__ hd, RRSel *__restrict__ sel) {
    __shared__ double part[256];
    const int t = threadIdx.x;
    const RRSel s = *sel;
    if (s.done) return;
    auto cnt = [&](int b) -> double { return hd ? hd[b] : (double)hist[b]; };
    if (s.single) {
        if (t == 0) {
            RRSel r = s;
            r.prefix = ((unsigned long long)cnt(RR_BINS) << 32) | (unsigned long long)cnt(RR_BINS + 1);
            r.pshift = 0;
            r.done = 1;
            r.single = 0;
            *sel = r;
        }
        __syncthreads();
        if (t < 2) hist[RR_BINS + t] = 0;
        return;
    }
    const int sh = digit_shift(s.pshift), nb = 1 << (s.pshift - sh);
    double c[8], sum = 0.0;
#pragma unroll
    for (int i = 0; i < 8; i++) {
        const int b = 8 * t + i;
        c[i] = b < nb ? cnt(b) : 0.0;
        sum += c[i];
    }
    part[t] = sum;
    __syncthreads();
    for (int off = 1; off < 256; off <<= 1) {   // inclusive scan of the threads' sums
        const double v = t >= off ? part[t - off] : 0.0;
        __syncthreads();
        part[t] += v;
        __syncthreads();
    }
    const double rank = (double)s.rank, incl = part[t], excl = incl - sum;
    if (excl <= rank && rank < incl) {   // exactly one thread holds the rank
        double before = excl;
        int d = 8 * t;
        double cd = 0.0;
#pragma unroll
        for (int i = 0; i < 8; i++) {
            if (rank < before + c[i]) { d = 8 * t + i; cd = c[i]; break; }
            before += c[i];
        }
        RRSel r = s;
        r.prefix = s.prefix | ((unsigned long long)d << sh);
        r.rank = s.rank - (unsigned long long)before;
        r.pshift = sh;
        r.done = sh == 0;
        r.single = !r.done && cd == 1.0;
        *sel = r;
    }
    __syncthreads();
    for (int b = t; b < nb; b += 256) hist[b] = 0;
}

__global__ void k_rr_tod(const uint32_t *__restrict__ hist, double *__restrict__ hd) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < RR_BINS + 2) hd[i] = (double)hist[i];
}

// ------------------------------------------------------------------------------------------------
// t = max(min_px, k_median * median) (k_median <= 0: min_px; both <= 0 or no rule: +inf); keep iff e_d <= t
__device__ __forceinline__ double rr_threshold(unsigned long long median_key, int has_rule, double k_median, double min_px) {
    if (!has_rule || (k_median <= 0.0 && min_px <= 0.0)) return INFINITY;
    if (k_median <= 0.0) return min_px;
    const double a = k_median * key_err(median_key);
    return a > min_px ? a : min_px;
}

__global__ void __launch_bounds__(256) k_rr_keep(const double *__restrict__ err, const int32_t *__restrict__ frame_obs_start, int F,
                                                 RRSel *__restrict__ sel, int has_rule, double k_median, double min_px, uint8_t *__restrict__ keep,
                                                 double *__restrict__ fstat, uint32_t *__restrict__ emptied) {
    const double t = rr_threshold(sel->prefix, has_rule, k_median, min_px);
    if (blockIdx.x == 0 && threadIdx.x == 0) sel->t = t;
    const int lane = threadIdx.x & 63, f = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (f >= F) return;
    const int o0 = frame_obs_start[f], o1 = frame_obs_start[f + 1];
    int rej = 0;
    for (int o = o0 + lane; o < o1; o += 64) {
        const bool k = err[o] <= t;
        keep[o] = k ? 1 : 0;
        rej += k ? 0 : 1;
    }
    rej = wave_sum_i(rej);
    if (lane == 0) {
        fstat[4 * (size_t)f + 3] = (double)rej;
        if (o1 > o0 && rej == o1 - o0) atomicAdd(emptied, 1u);
    }
}

// run record: {detections, sum r^2, rejected, non-finite, NaN} and the largest key
__global__ void __launch_bounds__(256) k_rr_runs(const double *__restrict__ err, const double *__restrict__ ss, const int32_t *__restrict__ perm,
                                                 const int32_t *__restrict__ run_start, int R, const RRSel *__restrict__ sel,
                                                 double *__restrict__ rstat, unsigned long long *__restrict__ rmax) {
    const int lane = threadIdx.x & 63, r = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= R) return;
    const double t = sel->t;
    const int j0 = run_start[r], j1 = run_start[r + 1];
    double sum = 0.0;
    int rej = 0, nf = 0, nn = 0;
    unsigned long long mk = 0;
    for (int j = j0 + lane; j < j1; j += 64) {
        const int o = perm[j];
        const double e = err[o];
        sum += ss[o];
        rej += (e <= t) ? 0 : 1;
        nf += isfinite(e) ? 0 : 1;
        nn += isnan(e) ? 1 : 0;
        const unsigned long long key = err_key(e);
        mk = key > mk ? key : mk;
    }
    sum = wave_sum_x(sum);
    rej = wave_sum_i(rej);
    nf = wave_sum_i(nf);
    nn = wave_sum_i(nn);
    mk = wave_max_k(mk);
    if (lane == 0) {
        double *q = rstat + 5 * (size_t)r;
        q[0] = (double)(j1 - j0); q[1] = sum; q[2] = (double)rej; q[3] = (double)nf; q[4] = (double)nn;
        rmax[r] = mk;
    }
}

// entity e < C: camera e (its runs are contiguous in ordering B); else marker e - C (its runs listed camera-ascending).
// esum[5 e ..] = {detections, sum r^2, rejected, non-finite, NaN}, emax[e] = largest e_d (NaN as +inf: esum carries the NaN count),
// esum[5 (C + M)] = frames emptied on this rank.  A communicator all-reduces esum (sum) and emax (max).
__global__ void __launch_bounds__(256) k_rr_entities(const double *__restrict__ rstat, const unsigned long long *__restrict__ rmax,
                                                     const int32_t *__restrict__ cam_run_start, const int32_t *__restrict__ mk_run_start,
                                                     const int32_t *__restrict__ mk_runs, int C, int M, const uint32_t *__restrict__ emptied,
                                                     double *__restrict__ esum, double *__restrict__ emax) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e == 0) esum[5 * (size_t)(C + M)] = (double)*emptied;
    if (e >= C + M) return;
    const bool cam = e < C;
    const int b = cam ? cam_run_start[e] : mk_run_start[e - C], n = (cam ? cam_run_start[e + 1] : mk_run_start[e - C + 1]) - b;
    double q[5] = {0, 0, 0, 0, 0};
    unsigned long long mk = 0;
    for (int i = 0; i < n; i++) {
        const int r = cam ? b + i : mk_runs[b + i];
#pragma unroll
        for (int k = 0; k < 5; k++) q[k] += rstat[5 * (size_t)r + k];
        mk = rmax[r] > mk ? rmax[r] : mk;
    }
#pragma unroll
    for (int k = 0; k < 5; k++) esum[5 * (size_t)e + k] = q[k];
    emax[e] = mk == NAN_KEY ? INFINITY : key_err(mk);
}

// ------------------------------------------------------------------------------------------------
void launch_rr_errors(const DeviceProblem &P, int which, const RRWork &w, unsigned long long rank, hipStream_t st) {
    const KTable kt = k_table(P, which);
    hipLaunchKernelGGL(k_rr_errors, dim3((unsigned)std::max(1, (P.F + 3) / 4)), dim3(256), 0, st, P.a_idx, P.a_uv, P.ent[which], kt.base, kt.stride,
                       P.frame_obs_start, P.F, P.A, P.half_size, P.res_f32, w.err, w.ss, w.fstat, w.hist, w.sel, rank);
}
void launch_rr_select_pass(const DeviceProblem &P, const RRWork &w, hipStream_t st) {
    const int64_t want = (P.N + 255) / 256;
    const unsigned grid = (unsigned)std::max<int64_t>(1, std::min<int64_t>(want, P.n_cus));
    hipLaunchKernelGGL(k_rr_hist, dim3(grid), dim3(256), 0, st, w.err, P.N, w.hist, w.sel);
}
void launch_rr_to_double(const RRWork &w, hipStream_t st) {
    hipLaunchKernelGGL(k_rr_tod, dim3((RR_BINS + 2 + 255) / 256), dim3(256), 0, st, w.hist, w.hd);
}
void launch_rr_pick(const RRWork &w, bool reduced, hipStream_t st) {
    hipLaunchKernelGGL(k_rr_pick, dim3(1), dim3(256), 0, st, w.hist, reduced ? w.hd : nullptr, w.sel);
}
void launch_rr_stats(const DeviceProblem &P, const RRWork &w, int has_rule, double k_median, double min_px, hipStream_t st) {
    hipLaunchKernelGGL(k_rr_keep, dim3((unsigned)std::max(1, (P.F + 3) / 4)), dim3(256), 0, st, w.err, P.frame_obs_start, P.F, w.sel, has_rule,
                       k_median, min_px, w.keep, w.fstat, w.hist + RR_BINS + 2);
    if (w.R > 0)
        hipLaunchKernelGGL(k_rr_runs, dim3((unsigned)((w.R + 3) / 4)), dim3(256), 0, st, w.err, w.ss, w.perm, w.run_start, w.R, w.sel, w.rstat, w.rmax);
    hipLaunchKernelGGL(k_rr_entities, dim3((unsigned)((P.C + P.M + 255) / 256)), dim3(256), 0, st, w.rstat, w.rmax, w.cam_run_start, w.mk_run_start,
                       w.mk_runs, P.C, P.M, w.hist + RR_BINS + 2, w.esum, w.emax);
}

}  // namespace aar
