// The start of a live-tracker frame that arrives as RAW detections: what apps/track.cpp does before track() --
// obtain_pose_estimations (IPPE on every detection) and init_object_transforms (the vote over the candidate object poses) -- in ONE launch of
// ONE workgroup on the ring slot the frame was just copied into.  Nothing is allocated, nothing is atomic; every store is a plain vector store.
//
// k_live_init, phases separated by workgroup barriers:
//   ippe        one thread per detection: undistortion (the P = K corners replace the raw ones in the slot's records, so that k_live_push reads
//               the floats the data-set path would), the two float-rounded IPPE poses, has2 = (double)e2 / (double)e1 < threshold
//   candidates  in the reference's order (the host's stable sort by marker, then camera, rides behind the records): first solution, then the
//               second when has2; positions by a workgroup prefix sum over 1 + has2; T and the j-side record by k_object_cands' arithmetic
//   vote        one thread per candidate i, T_i in registers, j ascending over all candidates: k_vote's sums.  A candidate with a non-finite
//               entry gets cost NaN and is left out of the others' sums (in a set of finite candidates nothing is left out)
//   argmin      per thread over its own candidates ascending, then a fixed tree: cost < best, equal costs to the lower index, NaN never wins
//   write       the winner's 3x4 -> (rvec, t); under LIVE_START_BEST wavefronts 0 and 1 evaluate the frame's E_f at the vote and at the
//               prediction; the start pose goes into the slot's header, the info record into the tracker's state
#include "geom.hpp"
#include "ippe_vote.hpp"
#include "kernels.h"
#include "track_eval.hpp"

namespace aar {

namespace {

constexpr int LI_THREADS = 256;

struct LiveInitShared {
    int scan[LI_THREADS];
    double bc[LI_THREADS];
    int bi[LI_THREADS];
    double zv[6], zp[6];     // the vote's pose, the prediction
    double Ev, Ep;           // E_f of the new frame at the two
};

__device__ __forceinline__ bool finite12(const double *p) {
    bool ok = true;
#pragma unroll
    for (int i = 0; i < 12; i++) ok = ok && isfinite(p[i]);
    return ok;
}

// The start of one frame by one workgroup of LI_THREADS threads: the kernels below call it.
__device__ __forceinline__ void live_init_body(const LiveInitArgs &a, LiveInitShared &s) {
    const int t = threadIdx.x, lane = t & 63, wv = __builtin_amdgcn_readfirstlane(t >> 6);
    const int n = a.n_det;
    char *recs = a.slot + LIVE_HDR_BYTES;
    const int *perm = reinterpret_cast<const int *>(recs + (size_t)LIVE_REC_BYTES * n);
    const CamTab *cams = reinterpret_cast<const CamTab *>(a.cams);
    double *hdr = reinterpret_cast<double *>(a.slot);

    // ---- ippe ----
    for (int d = t; d < n; d += LI_THREADS) {
        char *rec = recs + (size_t)LIVE_REC_BYTES * d;
        const ObsIdx id = *reinterpret_cast<const ObsIdx *>(rec);
        float4 *uvp = reinterpret_cast<float4 *>(rec + sizeof(ObsIdx));
        const float4 u0 = uvp[0], u1 = uvp[1];
        const float raw[8] = {u0.x, u0.y, u0.z, u0.w, u1.x, u1.y, u1.z, u1.w};
        float q[8], pk[8];
        d_undistort4(raw, cams[id.cam], q, pk);
        uvp[0] = make_float4(pk[0], pk[1], pk[2], pk[3]);
        uvp[1] = make_float4(pk[4], pk[5], pk[6], pk[7]);
        if (a.do_vote) {
            float e1, e2;
            d_ippe_square(a.hf, q, a.poses + 24LL * d, a.poses + 24LL * d + 12, e1, e2);
            a.has2[d] = ((double)e2 / (double)e1 < a.threshold) ? 1 : 0;
        }
    }
    __syncthreads();

    // ---- candidates ----
    int ncand = 0;
    if (a.do_vote) {
        for (int k0 = 0; k0 < n; k0 += LI_THREADS) {
            const int k = k0 + t;
            const int d = k < n ? perm[k] : 0;
            const int c = k < n ? 1 + a.has2[d] : 0;
            s.scan[t] = c;
            __syncthreads();
            for (int off = 1; off < LI_THREADS; off <<= 1) {   // inclusive prefix sum of the chunk
                const int v = t >= off ? s.scan[t - off] : 0;
                __syncthreads();
                s.scan[t] += v;
                __syncthreads();
            }
            const int pos = ncand + s.scan[t] - c;
            if (k < n) {
                const ObsIdx id = *reinterpret_cast<const ObsIdx *>(recs + (size_t)LIVE_REC_BYTES * d);
                const Aff T_cr = aff_load(a.Tcr + 12LL * id.cam), T_mr = aff_load(a.Tmr + 12LL * (id.marker - a.C));
                for (int sol = 0; sol < c; sol++) {
                    const int i = pos + sol;
                    object_cand(aff_load(a.poses + 24LL * d + 12 * sol), T_cr, T_mr, a.h, a.Tc + 12LL * i, a.BJ + 24LL * i);
                    a.fin[i] = (finite12(a.Tc + 12LL * i) && finite12(a.BJ + 24LL * i) && finite12(a.BJ + 24LL * i + 12)) ? 1 : 0;
                }
            }
            ncand += s.scan[LI_THREADS - 1];
            __syncthreads();
        }
    }

    // ---- vote ----
    const double px[4] = {-a.h, a.h, a.h, -a.h}, py[4] = {a.h, a.h, -a.h, -a.h};
    double best = DBL_MAX;   // as vote_sets: a cost must be below the largest double to win
    int at = -1;
    for (int i = t; i < ncand; i += LI_THREADS) {
        double T[12];
#pragma unroll
        for (int k = 0; k < 12; k++) T[k] = a.Tc[12LL * i + k];
        double acc = 0;
#pragma unroll 1
        for (int j = 0; j < ncand; j++) {
            if (!a.fin[j]) continue;
            acc += vote_term(T, a.BJ + 24LL * j, px, py);
        }
        if (!a.fin[i]) acc = NAN;
        a.cost[i] = acc;
        if (acc < best) { best = acc; at = i; }
    }

    // ---- argmin ----
    s.bc[t] = best;
    s.bi[t] = at;
    __syncthreads();
    for (int off = LI_THREADS / 2; off > 0; off >>= 1) {
        if (t < off) {
            const double c2 = s.bc[t + off];
            const int i2 = s.bi[t + off];
            if (i2 >= 0 && (c2 < s.bc[t] || (c2 == s.bc[t] && i2 < s.bi[t]))) { s.bc[t] = c2; s.bi[t] = i2; }
        }
        __syncthreads();
    }
    const int winner = s.bi[0];
    const double vote_cost = winner >= 0 ? s.bc[0] : 0.0;

    // ---- write ----
    const bool pred = a.has_init || a.has_prev;
    if (t == 0) {
        double zv[6] = {0, 0, 0, 0, 0, 0};
        if (winner >= 0) aff_to_pose6(a.Tc + 12LL * winner, zv);
#pragma unroll
        for (int k = 0; k < 6; k++) {
            s.zv[k] = zv[k];
            // (zprev may BE hdr, the motion model's prediction: it is read here, two barriers before the header is written below)
            s.zp[k] = a.has_init ? hdr[k] : (a.has_prev ? a.zprev[k] : 0.0);
        }
        s.Ev = 0.0;
        s.Ep = 0.0;
    }
    __syncthreads();
    const bool both = a.policy == LIVE_START_BEST && winner >= 0 && pred;
    if (both && wv < 2) {
        TrackArgs ta;
        ta.idx = nullptr; ta.uv = nullptr; ta.ent = a.ent; ta.Kmat = a.Kmat; ta.frame_obs_start = nullptr;
        ta.kstride = 9; ta.A = 0; ta.F = 1; ta.huber = a.huber; ta.h = a.h_track;
        ta.max_iters = 0; ta.min_error = ta.min_step_error_diff = ta.min_average_step_error_diff = ta.tau = 0.0;
        ta.z = nullptr; ta.iters_out = nullptr; ta.err_out = nullptr;
        double z[6], V[21], g[6];
#pragma unroll
        for (int k = 0; k < 6; k++) z[k] = wv == 0 ? s.zv[k] : s.zp[k];
        const double E = track_eval_range<false, LIVE_REC_BYTES, LIVE_REC_BYTES>(ta, recs, recs + sizeof(ObsIdx), 0, n, z, lane, V, g);
        if (lane == 0) {
            if (wv == 0) s.Ev = E; else s.Ep = E;
        }
    }
    __syncthreads();
    // the start: the vote where one was won -- under LIVE_START_BEST only when it is strictly cheaper than the prediction --, else pose_init,
    // else the previous estimate; -1: none
    int src = a.has_init ? 0 : (a.has_prev ? 1 : -1);
    if (winner >= 0 && (!both || s.Ev < s.Ep)) src = 2;
    if (t < 6) {
        const double v = src == 2 ? s.zv[t] : s.zp[t];
        hdr[t] = v;
        a.info[8 + t] = v;
    }
    if (t == 64) {
        a.info[0] = (double)a.do_vote; a.info[1] = (double)ncand; a.info[2] = (double)winner; a.info[3] = vote_cost;
        a.info[4] = (double)src; a.info[5] = s.Ep; a.info[6] = s.Ev; a.info[7] = 0.0; a.info[14] = 0.0; a.info[15] = 0.0;
    }
}

__global__ void __launch_bounds__(LI_THREADS) k_live_init(const LiveInitArgs a) {
    __shared__ LiveInitShared s;
    live_init_body(a, s);
}

__device__ __forceinline__ unsigned long long uni64(unsigned long long v) {
    const unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)v), hi = __builtin_amdgcn_readfirstlane((unsigned)(v >> 32));
    return ((unsigned long long)hi << 32) | lo;
}
template <typename T>
__device__ __forceinline__ T *uni_ptr(T *p) { return reinterpret_cast<T *>(uni64(reinterpret_cast<unsigned long long>(p))); }

// The bank: workgroup b starts member b's new frame.  The member's row of the table, the shared block and the new slot's
// header (detection count, whether it holds a pose_init) give its LiveInitArgs; everything is indexed by blockIdx.x alone.  A member's
// workspace slice is its own, so the workgroups of a launch share nothing but read-only tables.
__global__ void __launch_bounds__(LI_THREADS) k_live_init_bank(const LiveInitBankArgs ba) {
    __shared__ LiveInitShared s;
    const LiveInitMember *m = ba.tab + blockIdx.x;
    LiveInitArgs a;
    a.slot = ba.slot0 + (size_t)blockIdx.x * ba.slot_bytes;
    const double *hdr = reinterpret_cast<const double *>(a.slot);
    a.n_det = __builtin_amdgcn_readfirstlane((int)hdr[LIVE_HDR_CNT]);
    a.has_init = __builtin_amdgcn_readfirstlane((int)hdr[LIVE_HDR_INIT]);
    a.cams = uni_ptr(m->cams); a.Tcr = uni_ptr(m->Tcr); a.Tmr = uni_ptr(m->Tmr);
    a.C = __builtin_amdgcn_readfirstlane(m->C);
    a.hf = m->hf; a.h = m->h; a.threshold = m->threshold;
    a.policy = __builtin_amdgcn_readfirstlane(m->policy);
    // a vote is held unless the caller's pose_init settles the start (policy VOTE) or the frame has too few detections
    a.do_vote = (a.n_det >= __builtin_amdgcn_readfirstlane(m->min_detections) && !(a.has_init && a.policy == LIVE_START_VOTE)) ? 1 : 0;
    a.has_prev = ba.has_prev;
    a.zprev = ba.pred_in_header ? hdr : uni_ptr(m->zslot) + 6 * ba.prev_slot;
    a.ent = uni_ptr(m->ent); a.Kmat = uni_ptr(m->Kmat); a.huber = ba.huber; a.h_track = m->h_track;
    live_init_work_carve(a, uni_ptr(m->work), ba.max_obs);
    a.info = uni_ptr(m->info);
    live_init_body(a, s);
}

}  // namespace

void launch_live_init_bank(const LiveInitBankArgs &a, int B, hipStream_t st) {
    hipLaunchKernelGGL(k_live_init_bank, dim3(B), dim3(LI_THREADS), 0, st, a);
}

void launch_live_init(const LiveInitArgs &a, hipStream_t st) {
    hipLaunchKernelGGL(k_live_init, dim3(1), dim3(LI_THREADS), 0, st, a);
}

}  // namespace aar
