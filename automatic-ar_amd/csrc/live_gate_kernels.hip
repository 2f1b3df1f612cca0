// The gate of the live tracker: the batch path's outlier rule (aar_outlier_rule, include/aar.h) applied to the NEW frame
// of a push, at the pose the push starts from, in ONE launch of one workgroup per tracker between the frame's start and its refinement.  The
// refinement then reads a shorter frame: the same records, in the same order, as if the caller had left the rejected detections out.
//
// k_live_gate, phases separated by workgroup barriers:
//   errors      one thread per detection (d = t, t + 256, ...): e_d = sqrt((sum over the 4 corners of rx^2 + ry^2) / 4) at z0, track_eval's
//               double residuals, unweighted, summed in corner order -> det_err (the caller's order)
//   order       the e_d as 64-bit keys in LDS (the bits of a non-negative double order as the doubles do; a non-finite e_d takes +inf's bits,
//               the padding all ones), sorted by a bitonic network: exact, no sum in it.  median = key[(n - 1) / 2], max = key[n - 1]
//   threshold   t = max(min_px, k_median median), k_median <= 0: t = min_px; below min_detections the gate does not act: t = +inf, all kept
//   compaction  stable, in place, in ascending chunks of 256 records (see live_gate_compact)
//   record      the kept count into the slot header (LIVE_HDR_CNT, where k_live_push_bank reads it), the gate record, the keep flags
// No atomics, no scratch, nothing allocated; the only sums are the four corners of one detection and integer counts, so the result is the same
// bits in every run and in every bank size.
#include "geom.hpp"
#include "kernels.h"

namespace aar {

namespace {

constexpr int LG_THREADS = 256;
constexpr unsigned long long LG_KEY_INF = 0x7FF0000000000000ull, LG_KEY_PAD = ~0ull;

struct LiveGateShared {
    unsigned long long key[LIVE_GATE_MAX_OBS];
    int wsum[LG_THREADS / 64];   // a chunk's kept records by wavefront
    int nonfin[LG_THREADS / 64];
};

// what one workgroup needs of its tracker
struct LiveGateOne {
    char *slot;                  // header | n records
    int n, has_init;             // has_init: z0 is the header's pose, else zprev
    const double *zprev;
    const double *ent, *Kmat;
    double h;
    double *rec, *det_err;
    uint8_t *keep;
};

__device__ __forceinline__ bool lg_keep(double e, double thr, bool gated) { return !gated || (isfinite(e) && e <= thr); }

// Stable in-place compaction of the kept 48-byte records.  Record i goes to position (kept records before i) <= i, so a destination never lies
// above its source, but within one pass thread x may write a position that thread y has not read yet.  Hence chunks of LG_THREADS records in
// ascending order, each in two steps with a barrier between them: every thread READS its record of the chunk into registers, barrier, every
// kept record is WRITTEN.  That is enough because a write of chunk c lands in [base, base + kept of c) with base <= c LG_THREADS: either inside
// chunk c, whose records are all in registers by then, or in an earlier chunk, whose records were read in an earlier round (the barrier that
// ends a round orders them); never in a later chunk, which is still untouched when its turn comes.  Returns the kept count.
__device__ __forceinline__ int live_gate_compact(const LiveGateOne &a, LiveGateShared &s, double thr, bool gated) {
    const int t = threadIdx.x, lane = t & 63, wv = t >> 6, n = a.n;
    char *recs = a.slot + LIVE_HDR_BYTES;
    int base = 0;
    for (int c0 = 0; c0 < n; c0 += LG_THREADS) {
        const int i = c0 + t;
        const bool in = i < n;
        const bool k = in && lg_keep(a.det_err[i], thr, gated);   // (det_err[i]: this thread's own store of the first phase)
        if (in) a.keep[i] = k ? 1 : 0;
        const unsigned long long bal = __ballot(k);
        const int before = __popcll(bal & ((1ull << lane) - 1ull));
        if (lane == 0) s.wsum[wv] = __popcll(bal);
        uint4 r0 = make_uint4(0, 0, 0, 0), r1 = r0, r2 = r0;
        if (k) {
            const uint4 *src = reinterpret_cast<const uint4 *>(recs + (size_t)LIVE_REC_BYTES * i);
            r0 = src[0]; r1 = src[1]; r2 = src[2];
        }
        __syncthreads();   // the chunk is in registers, the counts in LDS
        int off = base + before, all = 0;
#pragma unroll
        for (int w = 0; w < LG_THREADS / 64; w++) {
            const int c = s.wsum[w];
            if (w < wv) off += c;
            all += c;
        }
        if (k && off != i) {
            uint4 *dst = reinterpret_cast<uint4 *>(recs + (size_t)LIVE_REC_BYTES * off);
            dst[0] = r0; dst[1] = r1; dst[2] = r2;
        }
        base += all;
        __syncthreads();   // the round's writes and its reads of the counts are done
    }
    return base;
}

__device__ __forceinline__ void live_gate_body(const LiveGateOne &a, const LiveGateParams &g, LiveGateShared &s) {
    const int t = threadIdx.x, lane = t & 63, wv = t >> 6, n = a.n;
    double *hdr = reinterpret_cast<double *>(a.slot);
    const char *recs = a.slot + LIVE_HDR_BYTES;

    // ---- errors ----
    int P = 2;
    while (P < n) P <<= 1;
    if (n > 0) {
        double z0[6], row[ENT_STRIDE];
#pragma unroll
        for (int k = 0; k < 6; k++) z0[k] = a.has_init ? hdr[k] : a.zprev[k];
        make_ent_row(z0, row);
        Ent ef;
#pragma unroll
        for (int i = 0; i < 9; i++) { ef.R[i] = row[i]; ef.Jl[i] = row[12 + i]; }
#pragma unroll
        for (int i = 0; i < 3; i++) ef.t[i] = row[9 + i];
        for (int d = t; d < P; d += LG_THREADS) {
            unsigned long long key = LG_KEY_PAD;
            if (d < n) {
                const char *rec = recs + (size_t)LIVE_REC_BYTES * d;
                const ObsIdx id = *reinterpret_cast<const ObsIdx *>(rec);
                const float4 uv0 = reinterpret_cast<const float4 *>(rec + sizeof(ObsIdx))[0];
                const float4 uv1 = reinterpret_cast<const float4 *>(rec + sizeof(ObsIdx))[1];
                const float ou[8] = {uv0.x, uv0.y, uv0.z, uv0.w, uv1.x, uv1.y, uv1.z, uv1.w};
                Ent ec, em;
                load_ent(a.ent, id.cam, ec);
                load_ent(a.ent, id.marker, em);
                double K[9];
#pragma unroll
                for (int i = 0; i < 9; i++) K[i] = a.Kmat[9 * id.cam + i];
                double sum = 0.0;
#pragma unroll
                for (int k = 0; k < 4; k++) {
                    CornerGeom gm;
                    project_corner(ec, em, ef, K, a.h, k, gm);
                    double rx, ry;
                    corner_residual(ou[2 * k], ou[2 * k + 1], gm.u, gm.v, 0, -1.f, rx, ry);
                    sum += rx * rx + ry * ry;
                }
                const double e = sqrt(sum / 4.0);
                a.det_err[d] = e;
                key = isfinite(e) ? (unsigned long long)__double_as_longlong(e) : LG_KEY_INF;
            }
            s.key[d] = key;
        }
    }
    __syncthreads();

    // ---- order ----
    double median = 0.0, mx = 0.0;
    int nonfinite = 0;
    if (n > 0) {
        for (int k = 2; k <= P; k <<= 1) {
            for (int j = k >> 1; j > 0; j >>= 1) {
                for (int i = t; i < P; i += LG_THREADS) {
                    const int l = i ^ j;
                    if (l > i) {
                        const unsigned long long x = s.key[i], y = s.key[l];
                        if ((x > y) == ((i & k) == 0)) { s.key[i] = y; s.key[l] = x; }
                    }
                }
                __syncthreads();
            }
        }
        median = __longlong_as_double((long long)s.key[(n - 1) / 2]);
        mx = __longlong_as_double((long long)s.key[n - 1]);
        int cnt = 0;
        for (int i0 = 0; i0 < n; i0 += LG_THREADS) cnt += __popcll(__ballot(i0 + t < n && s.key[i0 + t] >= LG_KEY_INF));
        if (lane == 0) s.nonfin[wv] = cnt;
        __syncthreads();
#pragma unroll
        for (int w = 0; w < LG_THREADS / 64; w++) nonfinite += s.nonfin[w];
    }

    // ---- threshold ----
    const bool gated = n >= g.min_detections;
    double thr = INFINITY;
    if (gated) thr = g.k_median > 0.0 ? fmax(g.min_px, g.k_median * median) : g.min_px;

    // ---- compaction ----
    const int kept = live_gate_compact(a, s, thr, gated);

    // ---- record ----
    if (t == 0) {
        hdr[LIVE_HDR_CNT] = (double)kept;
        a.rec[0] = gated ? 1.0 : 0.0; a.rec[1] = (double)n; a.rec[2] = (double)kept; a.rec[3] = (double)nonfinite;
        a.rec[4] = median; a.rec[5] = mx; a.rec[6] = thr; a.rec[7] = 0.0;
    }
}

__device__ __forceinline__ unsigned long long lg_uni64(unsigned long long v) {
    const unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)v), hi = __builtin_amdgcn_readfirstlane((unsigned)(v >> 32));
    return ((unsigned long long)hi << 32) | lo;
}
template <typename T>
__device__ __forceinline__ T *lg_uni_ptr(T *p) { return reinterpret_cast<T *>(lg_uni64(reinterpret_cast<unsigned long long>(p))); }

__global__ void __launch_bounds__(LG_THREADS) k_live_gate(const LiveGateArgs ga) {
    __shared__ LiveGateShared s;
    LiveGateOne a;
    a.slot = ga.slot; a.n = min(max(ga.n, 0), LIVE_GATE_MAX_OBS); a.has_init = ga.has_init; a.zprev = ga.zprev;
    a.ent = ga.ent; a.Kmat = ga.Kmat; a.h = ga.h; a.rec = ga.rec; a.det_err = ga.det_err; a.keep = ga.keep;
    live_gate_body(a, ga.g, s);
}

// The bank: workgroup b gates member b's new frame.  The count and whether the header holds a start pose come from the slot header, as in
// k_live_init_bank and k_live_push_bank; everything is indexed by blockIdx.x alone.
__global__ void __launch_bounds__(LG_THREADS) k_live_gate_bank(const LiveGateBankArgs ba) {
    __shared__ LiveGateShared s;
    const LiveGateMember *m = ba.tab + blockIdx.x;
    LiveGateOne a;
    a.slot = ba.slot0 + (size_t)blockIdx.x * ba.slot_bytes;
    const double *hdr = reinterpret_cast<const double *>(a.slot);
    a.n = min(max(__builtin_amdgcn_readfirstlane((int)hdr[LIVE_HDR_CNT]), 0), LIVE_GATE_MAX_OBS);
    a.has_init = ba.raw ? 1 : __builtin_amdgcn_readfirstlane((int)hdr[LIVE_HDR_INIT]);
    a.zprev = lg_uni_ptr(m->zslot) + 6 * ba.prev_slot;
    a.ent = lg_uni_ptr(m->ent); a.Kmat = lg_uni_ptr(m->Kmat); a.h = m->h;
    a.rec = lg_uni_ptr(m->rec); a.det_err = lg_uni_ptr(m->det_err); a.keep = lg_uni_ptr(m->keep);
    live_gate_body(a, ba.g, s);
}

}  // namespace

void launch_live_gate(const LiveGateArgs &a, hipStream_t st) { hipLaunchKernelGGL(k_live_gate, dim3(1), dim3(LG_THREADS), 0, st, a); }

void launch_live_gate_bank(const LiveGateBankArgs &a, int B, hipStream_t st) {
    hipLaunchKernelGGL(k_live_gate_bank, dim3(B), dim3(LG_THREADS), 0, st, a);
}

}  // namespace aar
