// C-ABI compute entry points (include/aar.h): problem upload, index structures, the LM loop of
// ucoslam::SparseLevMarq<double> (libs/sparselevmarq.h:238-249,349-430,440-472) driven from the host
// with every arithmetic stage on the GPU, and the RCCL exchange for frame-sharded problems.
//
// There is deliberately no CPU compute path in this file: without a HIP device every compute entry
// point returns AAR_ERR_NO_DEVICE.
#include <hip/hip_runtime.h>
#include <dlfcn.h>
#include <execinfo.h>
#include <fcntl.h>
#include <unistd.h>
#include <signal.h>

#include <algorithm>
#include <array>
#include <atomic>
#include <chrono>
#include <cmath>
#include <cstddef>
#include <cstring>
#include <map>
#include <memory>
#include <numeric>
#include <optional>
#include <condition_variable>
#include <mutex>
#include <vector>

#include "../host/internal.h"
#include "../host/se3.h"
#include "../host/motion_model.h"
#include "../host/problem_plan.h"
#include "geom.hpp"
#include "hostcopy.h"
#include "kernels.h"

using namespace aar;

#define HIP_TRY(expr)                                                                                  \
    do {                                                                                               \
        hipError_t _e = (expr);                                                                        \
        if (_e != hipSuccess) return set_error(AAR_ERR_HIP, "%s failed: %s", #expr, hipGetErrorString(_e)); \
    } while (0)

// kernels.h: the one record of the dynamic LDS each kernel may use on each device
void aar::raise_dynamic_lds(const void *kernel, size_t bytes) {
    constexpr size_t FLOOR = 48 * 1024;   // what every launcher asks for without an opt-in
    static std::mutex mu;
    static std::map<std::pair<int, const void *>, size_t> granted;
    if (bytes <= FLOOR) return;
    int dev = 0;
    (void)hipGetDevice(&dev);
    std::lock_guard<std::mutex> lock(mu);
    const auto key = std::make_pair(dev, kernel);
    const auto it = granted.find(key);
    if (it != granted.end() && it->second >= bytes) return;
    if (hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes) == hipSuccess) granted[key] = bytes;
    else (void)hipGetLastError();   // (not recorded: the launch that asks for it fails and reports its own error)
}

// ------------------------------------------------------------------------------------------------
// RCCL, resolved at run time so that libaar.so loads on machines without it (and shares whichever
// librccl.so.1 the process already holds, e.g. the one PyTorch brought in).
// ------------------------------------------------------------------------------------------------
namespace {
struct NcclId { char internal[128]; };
typedef void *NcclComm;
struct NcclApi {
    void *lib = nullptr;
    int (*GetUniqueId)(NcclId *) = nullptr;
    int (*CommInitRank)(NcclComm *, int, NcclId, int) = nullptr;
    int (*AllReduce)(const void *, void *, size_t, int, int, NcclComm, hipStream_t) = nullptr;
    int (*CommDestroy)(NcclComm) = nullptr;
    int (*CommCount)(NcclComm, int *) = nullptr;
    const char *(*GetErrorString)(int) = nullptr;
    bool ok = false;
};
NcclApi g_nccl;
constexpr int NCCL_FLOAT64 = 8, NCCL_SUM = 0, NCCL_MAX = 2;

int load_nccl() {
    if (g_nccl.ok) return AAR_OK;
    // One node, one process per GPU over xGMI: the bootstrap sockets can stay on loopback and there is no InfiniBand to
    // probe.  On hosts whose name does not resolve the default interface discovery has been seen to take minutes.
    // Both are only defaults: a caller's own environment wins.
    setenv("NCCL_SOCKET_IFNAME", "lo", 0);
    setenv("NCCL_IB_DISABLE", "1", 0);
    const char *names[] = {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"};
    for (const char *n : names) {
        g_nccl.lib = dlopen(n, RTLD_NOW | RTLD_GLOBAL);
        if (g_nccl.lib) break;
    }
    if (!g_nccl.lib) return set_error(AAR_ERR_COMM, "cannot dlopen librccl: %s", dlerror());
    g_nccl.GetUniqueId = (int (*)(NcclId *))dlsym(g_nccl.lib, "ncclGetUniqueId");
    g_nccl.CommInitRank = (int (*)(NcclComm *, int, NcclId, int))dlsym(g_nccl.lib, "ncclCommInitRank");
    g_nccl.AllReduce = (int (*)(const void *, void *, size_t, int, int, NcclComm, hipStream_t))dlsym(g_nccl.lib, "ncclAllReduce");
    g_nccl.CommDestroy = (int (*)(NcclComm))dlsym(g_nccl.lib, "ncclCommDestroy");
    g_nccl.CommCount = (int (*)(NcclComm, int *))dlsym(g_nccl.lib, "ncclCommCount");
    g_nccl.GetErrorString = (const char *(*)(int))dlsym(g_nccl.lib, "ncclGetErrorString");
    if (!g_nccl.GetUniqueId || !g_nccl.CommInitRank || !g_nccl.AllReduce || !g_nccl.CommDestroy)
        return set_error(AAR_ERR_COMM, "librccl lacks the expected nccl* symbols");
    g_nccl.ok = true;
    return AAR_OK;
}
}  // namespace

// In-process stand-in for a communicator (bring-up / tests): `world` host threads of ONE process, each with its own
// aar_problem on the SAME GPU, exchange through this group instead of RCCL.  Every rule of the sharded path (frame ranges,
// the all-reduces of S | rhs, of the step's scalars, of the initial diagonal, the final gather) runs unchanged; only the
// transport differs.  Lets the multi-rank logic be checked on a 1-GPU box.
struct aar_local_group {
    int world = 1;
    std::mutex m;
    std::condition_variable cv;
    int arrived = 0;
    unsigned long long gen = 0;
    std::vector<const double *> ptrs;
    bool broken = false;
    // false: a rank never arrived (it failed before its collective) -- the group is marked broken and every waiter returns,
    // as a communicator whose peer died would; a test must fail, not hang
    bool barrier() {
        std::unique_lock<std::mutex> lk(m);
        if (broken) return false;
        const unsigned long long g = gen;
        if (++arrived == world) { arrived = 0; gen++; cv.notify_all(); return true; }
        if (!cv.wait_for(lk, std::chrono::seconds(120), [&] { return gen != g || broken; }) || broken) {
            broken = true;
            cv.notify_all();
            return false;
        }
        return true;
    }
};

struct aar_comm {
    NcclComm comm = nullptr;
    int world = 1, rank = 0, device = 0;
    aar_local_group *local = nullptr;   // non-null: in-process group instead of RCCL
    double *tmp = nullptr;              // local transport: reduction scratch on the device
    size_t tmp_count = 0;
    int64_t allreduce_calls = 0, allreduce_bytes = 0, last_system_bytes = 0;   // aar_comm_get_stats
};

namespace {
__global__ void k_local_reduce(double *__restrict__ out, const double *const *__restrict__ in, int world, size_t count, int is_max) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= count) return;
    double v = in[0][i];
    for (int r = 1; r < world; r++) v = is_max ? fmax(v, in[r][i]) : v + in[r][i];   // fixed rank order: every rank gets the same bits
    out[i] = v;
}

// The reduced system travels as the PACKED lower triangle (only that half is ever produced or read): row i of S contributes its
// i + 1 leading entries, then the `extra` doubles that sit right behind S (rhs | g0 | the step's scalars).  grid.y = row
// (row n_pad = the extra part), dir 0 = pack, 1 = unpack.
__global__ void __launch_bounds__(256) k_pack_system(double *__restrict__ S, int n_pad, int extra, double *__restrict__ packed, int dir,
                                                     double *__restrict__ host, unsigned long long publish_seq, const int32_t *__restrict__ flags) {
    const int i = blockIdx.y, j = blockIdx.x * 256 + threadIdx.x;
    const size_t tri = (size_t)n_pad * (n_pad + 1) / 2;
    if (dir == 1 && publish_seq && i == n_pad && j == 0) {
        // the step's scalars go to the host from HERE, beside the unpacking (the host only reads the record; the next kernel it
        // queues is stream-ordered behind this one): tail[0..3] reduced over the ranks, tail[4..7] this rank's own
        const double *red = packed + tri + 2 * (size_t)n_pad, *own = S + (size_t)n_pad * n_pad + 2 * (size_t)n_pad;
        double sc[8];
#pragma unroll
        for (int q = 0; q < 8; q++) sc[q] = (q < extra - 2 * n_pad) ? red[q] : own[q];
        publish_host(sc, flags, host, publish_seq, /*flags_reduced=*/1);
    }
    if (i < n_pad) {
        if (j > i) return;
        double *a = S + (size_t)i * n_pad + j, *b = packed + (size_t)i * (i + 1) / 2 + j;
        if (dir == 0) *b = *a; else *a = *b;
    } else if (j < extra) {
        double *a = S + (size_t)n_pad * n_pad + j, *b = packed + tri + j;
        if (dir == 0) *b = *a; else *a = *b;
    }
}
}  // namespace

#define NCCL_TRY(expr)                                                                                          \
    do {                                                                                                        \
        int _r = (expr);                                                                                        \
        if (_r != 0)                                                                                            \
            return set_error(AAR_ERR_COMM, "%s failed: %s", #expr, g_nccl.GetErrorString ? g_nccl.GetErrorString(_r) : "?"); \
    } while (0)

// ------------------------------------------------------------------------------------------------
struct aar_problem {
    DeviceProblem P;
    PoseLayout L;             // global layout (all frames)
    int f_begin = 0, f_end = 0;  // global frame range owned by this rank
    int64_t o_begin = 0, N_global = 0;
    aar_comm *comm = nullptr;
    int device = 0;
    hipStream_t stream = nullptr;
    std::vector<void *> allocs;
    double *h_scal = nullptr;   // pinned, mapped [10]: 8 scalars | flags | sequence number (written by the device)
    int32_t h_flags[4] = {0, 0, 0, 0};
    unsigned long long seq = 0;
    double *d_frames_all = nullptr;  // [6 F_global] gather buffer (multi-GPU)
    double *d_diag = nullptr;        // [n_pad]
    double *d_pack = nullptr;        // multi-GPU: packed lower triangle of S | rhs | g0 | scalars, the all-reduce payload
    double *d_status = nullptr;      // multi-GPU: one double for collective status decisions
    PinnedBuf h_z;              // pose staging [6A + 6F_loc]: page-locked memory of the problem's own (hostcopy.h), so uploads need no sync
    double *h_gather = nullptr; size_t h_gather_n = 0;   // multi-rank: pinned landing zone of the gathered frame poses (download_z)
    hipEvent_t up_ev = nullptr;  // the last upload from h_z (it must have left before h_z is packed again)
    bool mu_seed_valid = false;  // max diag(J^T J) of the start point, published together with its sum r^2 (aar_lm_init)
    double mu_seed = 0;
    // host copies of the index structure (normal-equation assembly for tests)
    std::vector<int32_t> h_fslot_start, h_fslot_ent;
    std::vector<int32_t> h_ent_fixed;   // [A] the device's ent_fixed
    std::vector<aar_pose_prior> priors; // the caller's priors (aar_problem_constraints), in their order
    // LM state (SparseLevMarq members, libs/sparselevmarq.h:129-136)
    aar_lm_params prm;
    int cur = 0;                       // pose buffer / block set of curr_z
    double mu = -1, v = 2, currErr = 0, prevErr = 0;
    double rel_drop = -1;              // share of the error the last accepted LM step took away (-1: none yet); the PCG forcing sequence looks at it
    bool lm_ready = false;
    bool with_huber = false;
    float hubber_delta = 2.5f;         // MultiCamMapper::hubberDelta (libs/multicam_mapper.h:41)
    // SparseLevMarq::_step_callback / _stopFunction (libs/sparselevmarq.h:135-136)
    aar_lm_step_callback step_cb = nullptr;
    void *step_ctx = nullptr;
    bool step_want_z = false;
    aar_lm_stop_function stop_fn = nullptr;
    void *stop_ctx = nullptr;
    std::vector<double> cb_x, cb_z;    // staging of curr_z for the callbacks
    float huber_of_blocks = -1.f;      // Huber delta the residual behind blk[cur]'s B = -J^T r was weighted with (x64 of libs/sparselevmarq.h:367)
    bool blocks_valid = false;         // blk[cur] holds J^T J blocks and B at z[cur], S not yet eliminated
    double vinv_mu = -1;               // damping for which blk[cur].Vinv / hf are valid (< 0: none)
    double schur_mu = -1;              // damping whose Schur terms are already subtracted from blk[cur].S / rhs (< 0: none)
    int panels_blk = -1;               // MFMA Schur path: the block set whose dense panels Wd / Yd currently hold (-1: none) ...
    double panels_mu = -1;             // ... and the damping of the inverses behind Yd
    bool s_reduced = false;            // multi-GPU: blk[cur].S | rhs | g0 already hold the all-reduced system for schur_mu
    bool trial_reduced = false;        // ... the same for the trial's block set, until the step is accepted or rejected
    bool fused_comm = true;            // the step's scalars and the next step's system share ONE all-reduce (AAR_FUSED_COMM=0: two)
    // multi-GPU: the factorisation of the NEXT step's (already reduced) system is queued right behind the fused all-reduce, before the
    // host has seen this step's scalars -- the usual outcome (accepted, predicted damping) then finds it done, and the host's
    // turn-around hides behind it as it hides behind the Schur kernel on one GPU; any other outcome rebuilds the system anyway
    bool spec_chol = true;             // AAR_SPEC_CHOL=0: off
    int solver = AAR_SOLVER_DIRECT;    // what the problem runs with (aar_solver_options.solver, AUTO resolved)
    int env_overrides = 0;             // AAR_ENV_* bits: option fields an environment variable changed (aar_solver_stats.env_overrides)
    bool force_direct = false;         // solver spcg: THIS try takes the direct chain (the CG solve of the same system hit its cap / timed out)
    // ... and so do the next tries of this solve (the damping only falls along accepted steps: the systems get harder, not easier): 8 after the first
    // fall-back, twice as many after each further one (a 505-step -with-huber run moves its damping both ways: CG gets another chance now and then);
    // aar_lm_init clears both
    int spcg_skip = 0, spcg_backoff = 0;
    // CG iterations of the last SPCG solve of this LM run, as published with the step's scalars (-1: none yet).  Along an LM run the damping only falls and the systems only get
    // harder: a solve that came within 20 % of the iteration cap is taken as the announcement that the next one will not fit -- that try goes to the direct chain at once,
    // instead of through a failed CG attempt (64 .. 128 wasted iterations, the trial evaluation on a garbage step, a rebuild of the blocks)
    int last_cg_its = -1;
    int near_cap_tries = 0;            // tries the announcement above has sent to the direct chain: after 8 of them it is forgotten and the CG gets its chance again
    int64_t spcg_fallbacks = 0;
    double *h_pcg = nullptr;           // solver pcg with a communicator: pinned, mapped {done, iterations, -, sequence} the iteration launches publish
    unsigned long long pcg_seq = 0;
    int spec_chol_blk = -1;            // block set whose S a speculative factorisation has consumed (-1: none pending)
    double spec_chol_mu = -1;
    bool spec_chol_by_cg = false;      // ... whether it was a CG solve (a speculative solve is only consumed by a try that takes the same solver)
    double spec_chol_eta = 0;          // ... and the forcing term it was solved to (inexact solvers: a speculative solve is only consumed by a try that wants the same)
    hipStream_t stream2 = nullptr;     // download_z(side_stream): the copy of the final poses does not wait for the main stream
    bool merge_passes = true;          // passes A and B of an evaluation in one launch (AAR_MERGE_PASSES=0: two launches)
    int64_t trial_points = 0, launches = 0;
    aar_stage_times times;
    bool stage_timers = false;
    hipEvent_t ev[2] = {nullptr, nullptr};
    // per-kernel profiling (aar_set_kernel_profiling)
    bool profiling = false;
    std::vector<hipEvent_t> ev_pool;
    std::vector<int> ev_kid;       // kernel id of pending pair i (events 2i, 2i+1)
    size_t ev_used = 0;
    double k_seconds[KID_COUNT] = {0};
    int64_t k_launches[KID_COUNT] = {0};
    // aar_problem_covariance: workspace, allocated on the first call (cov_kernels.hip)
    double *cov_ws = nullptr;
    int32_t *cov_iws = nullptr;
    // aar_problem_residual_report: buffers and the ordering-B runs with their B -> A permutation, built on the first call (resid_kernels.hip)
    RRWork rr;
    bool rr_ready = false;
};

namespace {

template <class T>
int dev_alloc(aar_problem *pb, T **ptr, size_t count) {
    void *p = nullptr;
    size_t bytes = std::max<size_t>(count, 1) * sizeof(T);
    HIP_TRY(hipMalloc(&p, bytes));
    HIP_TRY(hipMemsetAsync(p, 0, bytes, pb->stream));
    pb->allocs.push_back(p);
    *ptr = static_cast<T *>(p);
    return AAR_OK;
}

// host <-> device through the library's page-locked staging (hostcopy.h): the runtime never sees a pageable pointer
int copy_h2d(aar_problem *pb, void *dst, const void *src, size_t bytes) {
    const char *what = "";
    const int e = h2d(dst, src, bytes, pb->stream, &what);
    return e ? set_error(AAR_ERR_HIP, "%s failed: %s", what, hipGetErrorString((hipError_t)e)) : AAR_OK;
}
int copy_d2h(aar_problem *pb, void *dst, const void *src, size_t bytes) {
    const char *what = "";
    const int e = d2h(dst, src, bytes, pb->stream, &what);
    return e ? set_error(AAR_ERR_HIP, "%s failed: %s", what, hipGetErrorString((hipError_t)e)) : AAR_OK;
}

template <class T>
int dev_upload(aar_problem *pb, T **ptr, const std::vector<T> &h) {
    int rc = dev_alloc(pb, ptr, h.size());
    if (rc) return rc;
    return h.empty() ? AAR_OK : copy_h2d(pb, *ptr, h.data(), h.size() * sizeof(T));
}

int ensure_device(int device_id) {
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess || n <= 0)
        return set_error(AAR_ERR_NO_DEVICE, "no HIP device available (%s); this library has no CPU path",
                         e == hipSuccess ? "device count 0" : hipGetErrorString(e));
    if (device_id < 0 || device_id >= n) return set_error(AAR_ERR_INVALID, "device_id %d out of range (%d devices)", device_id, n);
    HIP_TRY(hipSetDevice(device_id));
    return AAR_OK;
}

// x_full (reference packing, roots skipped) -> device pose vector [A entities | local frames]
void pack_z(const aar_problem *pb, const double *x_full, double *z) {
    const PoseLayout &L = pb->L;
    const int A = pb->P.A, F = pb->P.F;
    memset(z, 0, (size_t)6 * (A + F) * sizeof(double));
    for (int c = 0; c < L.C; c++)
        if (c != L.rc) memcpy(&z[6 * (size_t)c], x_full + L.full_cam0() + 6LL * L.cam_slot(c), 6 * sizeof(double));
    for (int m = 0; m < L.M; m++)
        if (m != L.rm) memcpy(&z[6 * (size_t)(L.C + m)], x_full + L.full_mk0() + 6LL * L.mk_slot(m), 6 * sizeof(double));
    if (F) memcpy(&z[6 * (size_t)A], x_full + L.full_fr0() + 6LL * pb->f_begin, (size_t)6 * F * sizeof(double));
    if (L.oi)   // intrinsics entity of camera c: (fx, cx, fy, cy, -, -); the distortion entries d0..d4 never reach the projection
        for (int c = 0; c < L.C; c++) memcpy(&z[6 * (size_t)(L.C + L.M + c)], x_full + L.full_intr0() + 9LL * c, 4 * sizeof(double));
}

int upload_z(aar_problem *pb, const double *x_full, int which) {
    if (pb->up_ev) HIP_TRY(hipEventSynchronize(pb->up_ev));   // the previous upload has left the staging buffer (it normally has long ago)
    const size_t cnt = (size_t)6 * (pb->P.A + pb->P.F);
    if (pb->h_z.reserve(cnt)) return set_error(AAR_ERR_HIP, "hipHostMalloc(pose staging) failed");
    pack_z(pb, x_full, pb->h_z.data());
    if (!pb->up_ev && hipEventCreateWithFlags(&pb->up_ev, hipEventDisableTiming) != hipSuccess) { pb->up_ev = nullptr; (void)hipGetLastError(); }
    if (cnt) HIP_TRY(hipMemcpyAsync(pb->P.z[which], pb->h_z.data(), cnt * sizeof(double), hipMemcpyHostToDevice, pb->stream));   // (page-locked source)
    if (pb->up_ev) HIP_TRY(hipEventRecord(pb->up_ev, pb->stream));
    else HIP_TRY(hipStreamSynchronize(pb->stream));
    return AAR_OK;
}

int allreduce(aar_problem *pb, double *buf, size_t count, int op) {
    if (!pb->comm) return AAR_OK;
    pb->comm->allreduce_calls++;
    pb->comm->allreduce_bytes += (int64_t)(count * sizeof(double));
    if (aar_local_group *g = pb->comm->local) {   // in-process transport (see aar_local_group)
        aar_comm *c = pb->comm;
        if (c->tmp_count < count + (size_t)g->world) {
            if (c->tmp) (void)hipFree(c->tmp);
            c->tmp_count = count + (size_t)g->world;
            HIP_TRY(hipMalloc((void **)&c->tmp, c->tmp_count * sizeof(double)));
        }
        HIP_TRY(hipStreamSynchronize(pb->stream));            // my contribution is complete
        g->ptrs[c->rank] = buf;
        if (!g->barrier()) return set_error(AAR_ERR_COMM, "local group: a rank did not reach the collective");   // ... and so is everybody else's
        const double **d_ptrs = reinterpret_cast<const double **>(c->tmp + count);
        { int rc = copy_h2d(pb, (void *)d_ptrs, g->ptrs.data(), sizeof(double *) * g->world); if (rc) return rc; }
        hipLaunchKernelGGL(k_local_reduce, dim3((unsigned)((count + 255) / 256)), dim3(256), 0, pb->stream, c->tmp, d_ptrs, g->world, count,
                           op == NCCL_MAX ? 1 : 0);
        HIP_TRY(hipStreamSynchronize(pb->stream));
        if (!g->barrier()) return set_error(AAR_ERR_COMM, "local group: a rank did not reach the collective");   // everyone has read everyone's buffer: it may be overwritten now
        HIP_TRY(hipMemcpyAsync(buf, c->tmp, count * sizeof(double), hipMemcpyDeviceToDevice, pb->stream));
        return AAR_OK;
    }
    NCCL_TRY(g_nccl.AllReduce(buf, buf, count, NCCL_FLOAT64, op, pb->comm->comm, pb->stream));
    return AAR_OK;
}

// All-reduce of the reduced system of block set `which`: packed lower triangle of S | rhs | g0 (| the first n_tail doubles of
// the tail: the step's scalars of the fused collective).  n_pad (n_pad + 1) / 2 + 2 n_pad + n_tail doubles instead of the
// n_pad^2 + ... of the square.
int allreduce_system(aar_problem *pb, int which, int n_tail, unsigned long long publish_seq = 0) {
    DeviceProblem &P = pb->P;
    // Small systems travel as they lie -- the square S (its upper triangle is never written: zeros) | rhs | g0 | tail are ONE allocation --
    // without the two packing launches: below ~1 MB an all-reduce over xGMI is latency, not bytes, and each launch on this dependent
    // chain costs 3-4 us.  From 384 unknowns on (2.4 MB square) the packed triangle's halved payload wins.  AAR_PACK_SYSTEM=0 / 1 forces.
    const bool pack = P.tune.pack_system >= 0 ? P.tune.pack_system != 0 : P.n_pad > 384;
    if (!pack) {
        const size_t count = (size_t)P.n_pad * P.n_pad + 2 * (size_t)P.n_pad + (size_t)n_tail;
        int rc = allreduce(pb, P.blk[which].S, count, NCCL_SUM);
        if (rc) return rc;
        pb->comm->last_system_bytes = (int64_t)(count * sizeof(double));
        // tail[0..3] are now the rank sums, tail[4..7] still this rank's own: exactly the record the host reads
        if (publish_seq) { launch_publish(P, publish_seq, pb->stream, P.blk[which].tail, /*flags_reduced=*/true); pb->launches += 1; }
        return AAR_OK;
    }
    const int extra = 2 * P.n_pad + n_tail;
    const size_t count = (size_t)P.n_pad * (P.n_pad + 1) / 2 + (size_t)extra;
    const dim3 grid((unsigned)((std::max(P.n_pad, extra) + 255) / 256), (unsigned)P.n_pad + 1);
    hipLaunchKernelGGL(k_pack_system, grid, dim3(256), 0, pb->stream, P.blk[which].S, P.n_pad, extra, pb->d_pack, 0, nullptr, 0ull, nullptr);
    int rc = allreduce(pb, pb->d_pack, count, NCCL_SUM);
    if (rc) return rc;
    pb->comm->last_system_bytes = (int64_t)(count * sizeof(double));
    hipLaunchKernelGGL(k_pack_system, grid, dim3(256), 0, pb->stream, P.blk[which].S, P.n_pad, extra, pb->d_pack, 1, P.host_result, publish_seq, P.flags);
    pb->launches += 2;
    return AAR_OK;
}

// The same status on every rank: the most severe (most negative) code any rank holds.  A rank that fails alone would leave
// the others waiting in their next collective forever (RCCL has no timeout), so rank-local failures that decide control flow
// are agreed on first.
int collective_status(aar_problem *pb, int local_rc, int *agreed) {
    *agreed = local_rc;
    if (!pb->comm) return AAR_OK;
    const double v = (double)(-local_rc);
    int rc = copy_h2d(pb, pb->d_status, &v, sizeof v);
    if (rc) return rc;
    if ((rc = allreduce(pb, pb->d_status, 1, NCCL_MAX))) return rc;
    double w = 0;
    if ((rc = copy_d2h(pb, &w, pb->d_status, sizeof w))) return rc;
    *agreed = -(int)w;
    return AAR_OK;
}

// device pose vector -> x_full; fixed groups keep the caller's values
// side_stream: the copy goes through the problem's second stream and only THAT is waited for.  z[which] must be complete already (the host has
// seen the scalars of the step that wrote it); what is still running on the main stream -- the speculative Schur complement of a step that
// turned out to be the last, ~20 us -- then overlaps with the caller's own work instead of being waited for.  Single GPU only.
int download_z(aar_problem *pb, int which, double *x_full, bool side_stream = false) {
    const PoseLayout &L = pb->L;
    const int A = pb->P.A, F = pb->P.F;
    if (pb->up_ev) HIP_TRY(hipEventSynchronize(pb->up_ev));   // (the staging buffer is shared with the uploads)
    const size_t zcnt = (size_t)6 * (A + F);
    if (pb->h_z.reserve(zcnt)) return set_error(AAR_ERR_HIP, "hipHostMalloc(pose staging) failed");
    const double *z = pb->h_z.data();
    hipStream_t st = (side_stream && !pb->comm && pb->stream2) ? pb->stream2 : pb->stream;
    if (zcnt) HIP_TRY(hipMemcpyAsync(pb->h_z.data(), pb->P.z[which], zcnt * sizeof(double), hipMemcpyDeviceToHost, st));   // (page-locked destination)
    HIP_TRY(hipStreamSynchronize(st));
    if (L.oc)
        for (int c = 0; c < L.C; c++)
            if (c != L.rc) memcpy(x_full + L.full_cam0() + 6LL * L.cam_slot(c), &z[6 * (size_t)c], 6 * sizeof(double));
    if (L.om)
        for (int m = 0; m < L.M; m++)
            if (m != L.rm) memcpy(x_full + L.full_mk0() + 6LL * L.mk_slot(m), &z[6 * (size_t)(L.C + m)], 6 * sizeof(double));
    if (L.oi)
        for (int c = 0; c < L.C; c++) memcpy(x_full + L.full_intr0() + 9LL * c, &z[6 * (size_t)(L.C + L.M + c)], 4 * sizeof(double));
    if (L.of) {
        if (!pb->comm) {
            if (F) memcpy(x_full + L.full_fr0(), &z[6 * (size_t)A], (size_t)6 * F * sizeof(double));
        } else {
            // every rank contributes its own frames to a zeroed vector; the sum is the gather
            const size_t cnt = (size_t)6 * L.F;
            HIP_TRY(hipMemsetAsync(pb->d_frames_all, 0, cnt * sizeof(double), pb->stream));
            if (F)
                HIP_TRY(hipMemcpyAsync(pb->d_frames_all + 6 * (size_t)pb->f_begin, pb->P.z[which] + 6 * (size_t)A,
                                       (size_t)6 * F * sizeof(double), hipMemcpyDeviceToDevice, pb->stream));
            int rc = allreduce(pb, pb->d_frames_all, cnt, NCCL_SUM);
            if (rc) return rc;
            if (pb->h_gather_n < cnt) {   // (the caller's vector is pageable: the copy lands in pinned memory of the problem's own, allocated once)
                if (pb->h_gather) (void)hipHostFree(pb->h_gather);
                pb->h_gather = nullptr; pb->h_gather_n = 0;
                HIP_TRY(hipHostMalloc((void **)&pb->h_gather, cnt * sizeof(double), hipHostMallocDefault));
                pb->h_gather_n = cnt;
            }
            HIP_TRY(hipMemcpyAsync(pb->h_gather, pb->d_frames_all, cnt * sizeof(double), hipMemcpyDeviceToHost, pb->stream));
            HIP_TRY(hipStreamSynchronize(pb->stream));
            memcpy(x_full + L.full_fr0(), pb->h_gather, cnt * sizeof(double));
        }
    }
    return AAR_OK;
}

void prof_pre(void *ctx, int kid) {
    aar_problem *pb = static_cast<aar_problem *>(ctx);
    if (pb->ev_used + 2 > pb->ev_pool.size()) {
        hipEvent_t a, b;
        (void)hipEventCreate(&a);
        (void)hipEventCreate(&b);
        pb->ev_pool.push_back(a);
        pb->ev_pool.push_back(b);
    }
    pb->ev_kid.push_back(kid);
    (void)hipEventRecord(pb->ev_pool[pb->ev_used], pb->stream);
}
void prof_post(void *ctx, int) {
    aar_problem *pb = static_cast<aar_problem *>(ctx);
    (void)hipEventRecord(pb->ev_pool[pb->ev_used + 1], pb->stream);
    pb->ev_used += 2;
}
// after a stream synchronisation: fold the pending event pairs into the per-kernel totals
void prof_harvest(aar_problem *pb) {
    if (!pb->profiling) return;
    for (size_t i = 0; i < pb->ev_kid.size(); i++) {
        float ms = 0;
        if (hipEventElapsedTime(&ms, pb->ev_pool[2 * i], pb->ev_pool[2 * i + 1]) == hipSuccess) {
            pb->k_seconds[pb->ev_kid[i]] += ms * 1e-3;
            pb->k_launches[pb->ev_kid[i]]++;
        }
    }
    pb->ev_kid.clear();
    pb->ev_used = 0;
}

struct StageTimer {  // optional per-stage device timing (AAR_STAGE_TIMERS=1); costs two event records + a sync per stage
    aar_problem *pb;
    double *slot;
    StageTimer(aar_problem *p, double *s) : pb(p), slot(s) {
        if (pb->stage_timers) (void)hipEventRecord(pb->ev[0], pb->stream);
    }
    ~StageTimer() {
        if (pb->stage_timers) {
            (void)hipEventRecord(pb->ev[1], pb->stream);
            (void)hipEventSynchronize(pb->ev[1]);
            float ms = 0;
            (void)hipEventElapsedTime(&ms, pb->ev[0], pb->ev[1]);
            *slot += ms * 1e-3;
        }
    }
};

int check_async(const char *what) {
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return set_error(AAR_ERR_HIP, "%s: %s", what, hipGetErrorString(e));
    return AAR_OK;
}

// both block sets' shared system and the linear-model partials in ONE launch (aar_lm_init: seven hipMemsetAsync = seven fill
// kernels otherwise, ~25 us of a solve's fixed cost)
struct ZeroArgs { double *p[7]; long long n[7]; };
__global__ void __launch_bounds__(256) k_zero_many(const ZeroArgs z) {
    const long long gid = (long long)blockIdx.x * 256 + threadIdx.x, stride = (long long)gridDim.x * 256;
#pragma unroll
    for (int b = 0; b < 7; b++)
        for (long long i = gid; i < z.n[b]; i += stride) z.p[b][i] = 0.0;
}

int zero_for_init(aar_problem *pb) {
    DeviceProblem &P = pb->P;
    ZeroArgs z;
    const long long n2 = (long long)P.n_pad * P.n_pad;
    z.p[0] = P.blk[0].S; z.n[0] = n2; z.p[1] = P.blk[1].S; z.n[1] = n2;
    z.p[2] = P.blk[0].rhs; z.n[2] = P.n_pad; z.p[3] = P.blk[1].rhs; z.n[3] = P.n_pad;
    z.p[4] = P.blk[0].g0; z.n[4] = P.n_pad; z.p[5] = P.blk[1].g0; z.n[5] = P.n_pad;
    z.p[6] = P.lin_part; z.n[6] = 2LL * (P.F + 1);
    const long long blocks = std::min<long long>(2048, (2 * n2 + 255) / 256 + 1);
    hipLaunchKernelGGL(k_zero_many, dim3((unsigned)blocks), dim3(256), 0, pb->stream, z);
    pb->launches += 1;
    return check_async("k_zero_many");
}

int zero_block_set(aar_problem *pb, int which) {
    DeviceProblem &P = pb->P;
    HIP_TRY(hipMemsetAsync(P.blk[which].S, 0, (size_t)P.n_pad * P.n_pad * sizeof(double), pb->stream));
    HIP_TRY(hipMemsetAsync(P.blk[which].rhs, 0, (size_t)P.n_pad * sizeof(double), pb->stream));
    HIP_TRY(hipMemsetAsync(P.blk[which].g0, 0, (size_t)P.n_pad * sizeof(double), pb->stream));
    return AAR_OK;
}

// MFMA Schur path: do Wd / Yd already hold block set `which` for damping mu (pass A wrote them, or an earlier k_schur_fill)?
bool panels_ok(const aar_problem *pb, int which, double mu) { return pb->P.n_smwork > 0 && pb->panels_blk == which && pb->panels_mu == mu; }
// a Schur launch for (which, mu) leaves the panels behind for exactly that pair
void panels_now(aar_problem *pb, int which, double mu) { if (pb->P.n_smwork > 0) { pb->panels_blk = which; pb->panels_mu = mu; } }

// J^T J blocks and B at z[which] into blk[which] (whose S, rhs, g0 must be zero): the "J", "transpose", "Jt*J", "B"
// stages of libs/sparselevmarq.h:353-367.  Pass A also leaves the per-frame sums of r^2 in err_part and, for
// mu_pred >= 0, (V_f + mu_pred I)^-1; zero_blk >= 0 clears that block set on the way.
int eval_blocks(aar_problem *pb, int which, double mu_pred, int zero_blk, bool ents_ready = false) {
    DeviceProblem &P = pb->P;
    if (!ents_ready) launch_unpack(P, which, pb->stream);   // {R, t, J_l} rows of z[which]; after a damped try k_backsub has written them
    if (P.F == 0 && zero_blk >= 0) {  // a rank without frames launches no pass A: clear the dead block set here
        int rc = zero_block_set(pb, zero_blk);
        if (rc) return rc;
    }
    // pass A rewrites W of this block set: its old panels are stale; it writes new ones itself when it inverts V_f (mu_pred >= 0)
    if (pb->panels_blk == which) pb->panels_blk = -1;
    if (P.n_smwork > 0 && P.dense_from_passA && mu_pred >= 0.0 && P.F > 0) panels_now(pb, which, mu_pred);
    {
        StageTimer t(pb, &pb->times.jacobian_normal_eq);
        if (pb->merge_passes && launch_passAB(P, which, mu_pred, zero_blk, pb->stream)) {
            launch_prior(P, which, true, pb->stream);   // (priors: after pass B, before anything reads S)
            launch_pair_prior(P, which, true, pb->stream);
            pb->launches += 1 + n_prior_launches(P);
            return check_async("normal-equation kernels");
        }
        launch_passA(P, which, mu_pred, zero_blk, pb->stream);
        launch_passB(P, which, pb->stream);
        launch_prior(P, which, true, pb->stream);
        launch_pair_prior(P, which, true, pb->stream);
    }
    pb->launches += 2 + n_prior_launches(P);
    return check_async("normal-equation kernels");
}

// Wait for the device to publish record `seq` into the mapped host buffer.  Spinning on the sequence word avoids the
// two blit kernels and the interrupt latency of memcpy + hipStreamSynchronize on the per-try critical path.
int wait_result(aar_problem *pb) {
    volatile unsigned long long *sq = reinterpret_cast<volatile unsigned long long *>(pb->h_scal) + 9;
    const auto t0 = std::chrono::steady_clock::now();
    unsigned spins = 0;
    while (*sq != pb->seq) {
        if ((++spins & 0x3fff) == 0) {
            if (hipStreamQuery(pb->stream) == hipSuccess && *sq != pb->seq) {
                // the stream drained but the record is stale: an asynchronous failure
                hipError_t e = hipGetLastError();
                return set_error(AAR_ERR_HIP, "device did not publish its result: %s", hipGetErrorString(e));
            }
            if (std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count() > 120.0)
                return set_error(AAR_ERR_HIP, "timed out waiting for the device result");
        }
        __builtin_ia32_pause();
    }
    std::atomic_thread_fence(std::memory_order_acquire);
    pb->h_flags[0] = (int32_t)reinterpret_cast<volatile long long *>(pb->h_scal)[8];
    if (pb->profiling || pb->stage_timers) {
        HIP_TRY(hipStreamSynchronize(pb->stream));
        prof_harvest(pb);
    }
    return AAR_OK;
}

// queue the reduction of the step's scalars and their publication to the host record (no wait)
int launch_scalars(aar_problem *pb, int n_err, int maxdiag_blk = -1) {
    DeviceProblem &P = pb->P;
    pb->seq++;
    {
        StageTimer t(pb, &pb->times.control);
        // (PCG mode with ranks: g0 is this rank's partial sum -- it was never all-reduced --, so delta_s . g0 joins the rank sum)
        launch_reduce_scalars(P, n_err, P.use_pcg && pb->comm, pb->comm ? 0ull : pb->seq, pb->stream, nullptr, maxdiag_blk);
        pb->launches += 1;
    }
    if (pb->comm) {
        StageTimer t(pb, &pb->times.allreduce);
        int rc = allreduce(pb, P.scal, 4, NCCL_SUM);  // [sum r^2, sum |delta_f|^2, sum delta.g, every rank's error flags]
        if (rc) return rc;
        launch_publish(P, pb->seq, pb->stream, nullptr, /*flags_reduced=*/true);
    }
    return check_async("kernel launch");
}

int read_scalars(aar_problem *pb, int n_err, int maxdiag_blk = -1) {
    int rc = launch_scalars(pb, n_err, maxdiag_blk);
    if (rc) return rc;
    return wait_result(pb);
}

// One damped solve from blk[cur] (valid, un-eliminated) and the evaluation of the trial point:
//   Schur complement -> [all-reduce] -> LDL^T -> back-substitution -> z[1-cur] = z[cur] + delta
//   -> pass A / pass B at the trial point into blk[1-cur] (speculative: they ARE the next step's Jacobian pass when the
//      trial is accepted, and the trial's sum r^2 comes out of pass A) -> scalars to the host.
// blk[cur].S/rhs are consumed; pass A clears them together with blk[cur].g0 on the way.
constexpr int TRY_NOT_POSITIVE_DEFINITE = 1;   // damped_try: not an error code of the C ABI (those are negative)
constexpr int TRY_CG_FAILED = 2;               // solver spcg: the CG solve hit its iteration cap or its hand-over timed out; S is intact, the caller redoes the try with the direct chain

int damped_try(aar_problem *pb, double mu, bool evaluate_trial) {
    DeviceProblem &P = pb->P;
    const int cur = pb->cur, tr = 1 - cur;
    bool chol_done = false;
    const bool cg_near_cap = pb->last_cg_its >= 0 && 10 * pb->last_cg_its >= 8 * std::min(P.spcg_max_it, SPCG_MAX_IT);
    const bool by_cg = P.use_spcg && !pb->force_direct && pb->spcg_skip == 0 && !cg_near_cap;
    // the coarse space of the CG (k_spcg_pre + the roots' wavefronts) costs ~8 us per solve and saves iterations only once block-Jacobi needs many: it joins when a
    // solve of this run has taken spcg_coarse_from iterations and stays (the damping only falls from there on)
    if (!P.spcg_coarse_on && spcg_coarse_now(P) && (P.spcg_coarse_from <= 0 || pb->last_cg_its >= P.spcg_coarse_from)) P.spcg_coarse_on = 1;
    if (pb->spec_chol_blk >= 0) {   // a factorisation was queued ahead of the host's decision (multi-GPU, see aar_problem::spec_chol)
        if (pb->spec_chol_blk == cur && pb->spec_chol_mu == mu && pb->schur_mu == mu && pb->s_reduced && pb->spec_chol_by_cg == by_cg &&
            (!by_cg || pb->spec_chol_eta == P.pcg_eta_now)) {
            chol_done = true;       // the step was accepted with the predicted damping: this try's factorisation is already running
        } else {
            // rejected (the trial's block set is rebuilt from scratch) or accepted with another damping (s_reduced: the system is
            // rebuilt from the blocks below): what the speculative factorisation left in S, and in the pivot flags, means nothing
            HIP_TRY(hipMemsetAsync(P.flags, 0, 4 * sizeof(int32_t), pb->stream));
        }
        pb->spec_chol_blk = -1;
    }
    if (P.use_pcg) {   // opt-in: no Schur complement, no factorisation -- PCG through the frame blocks (pcg_kernels.hip)
        if (pb->vinv_mu != mu) {
            launch_frame_inv(P, cur, mu, pb->stream);
            pb->vinv_mu = mu;
            pb->launches += 1;
        }
        if (!pb->comm) {
            StageTimer t(pb, &pb->times.chol);
            launch_pcg(P, cur, mu, pb->stream);
            pb->launches += 1;
        } else {
            // frames sharded over ranks: the set-up shares and every iteration's partial y are all-reduced between launches; every
            // fourth launch publishes {done, iterations} so that the host stops queueing (all ranks read the same: same control flow)
            { StageTimer t(pb, &pb->times.chol); launch_pcgd_setup(P, cur, mu, pb->stream); }
            { StageTimer t(pb, &pb->times.allreduce); int rc = allreduce(pb, P.pcgd_setup, (size_t)P.A * 28 + ((P.pcg_fused && !P.deterministic && P.pcg_coarse) ? 144 : 0), NCCL_SUM); if (rc) return rc; }   // (+ the coarse operator's shares)
            pb->launches += 1;
            for (int k = 0;; k++) {
                const bool last = k >= P.pcg_max_it + 1;
                const bool poll = last || (k % 4) == 3;
                if (poll) pb->pcg_seq++;
                { StageTimer t(pb, &pb->times.chol); launch_pcgd_iter(P, cur, mu, k, last, poll ? pb->pcg_seq : 0ull, pb->stream); }
                pb->launches += 1;
                if (poll) {
                    int rc = check_async("pcg launch");
                    if (rc) return rc;
                    volatile unsigned long long *sq = reinterpret_cast<volatile unsigned long long *>(pb->h_pcg) + 3;
                    const auto t0 = std::chrono::steady_clock::now();
                    unsigned spins = 0;
                    int poll_rc = AAR_OK;
                    while (*sq != pb->pcg_seq) {
                        if ((++spins & 0x3fff) == 0) {
                            if (hipStreamQuery(pb->stream) == hipSuccess && *sq != pb->pcg_seq) {   // the stream drained but the record is stale: an asynchronous failure
                                poll_rc = set_error(AAR_ERR_HIP, "device did not publish the PCG progress record: %s", hipGetErrorString(hipGetLastError()));
                                break;
                            }
                            if (std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count() > 120.0) {
                                poll_rc = set_error(AAR_ERR_HIP, "timed out waiting for the PCG progress record");
                                break;
                            }
                        }
                        __builtin_ia32_pause();
                    }
                    std::atomic_thread_fence(std::memory_order_acquire);
                    // (a rank whose device has faulted or hangs cannot tell the others: its stream carries nothing any more, and an agreement per poll --
                    //  one more collective -- would cost every healthy step ~50 us; the peers then sit in their next all-reduce until the launcher's
                    //  watchdog ends the job, as with any rank that dies mid-collective)
                    if (poll_rc) return poll_rc;
                    if (pb->h_pcg[0] != 0.0 || last) break;
                }
                { StageTimer t(pb, &pb->times.allreduce); int rc = allreduce(pb, pcgd_y_of_launch(P, k), (size_t)6 * P.A, NCCL_SUM); if (rc) return rc; }
            }
        }
        chol_done = true;
    }
    if (!P.use_pcg && pb->schur_mu != mu) {  // not already done speculatively by the try that produced this point
        StageTimer t(pb, &pb->times.schur);
        if (pb->s_reduced) {
            // multi-GPU, fused collective: S | rhs | g0 of this point already hold the ALL-REDUCED system for the predicted
            // damping, so the terms cannot be taken back rank by rank.  Rebuild this rank's shared blocks from its observations
            // (pass B alone: the frame blocks V, W, g_f of pass A are untouched) -- a mispredicted damping is rare.
            int rc = zero_block_set(pb, cur);
            if (rc) return rc;
            launch_passB(P, cur, pb->stream);
            launch_prior(P, cur, true, pb->stream);
            launch_pair_prior(P, cur, true, pb->stream);
            pb->launches += 1 + n_prior_launches(P);
            pb->s_reduced = false;
        } else if (pb->schur_mu >= 0) {
            // the speculative Schur complement was taken with another damping than the step now needs (gain < 0.94): take it
            // back with the inverses it used (still in Vinv), keeping the blocks -- and the residual they were built from --
            // exactly those of the accepted trial, as the reference's x64 / J are
            launch_schur(P, cur, -1.0, pb->stream, 0, 0, nullptr, panels_ok(pb, cur, pb->schur_mu));
            panels_now(pb, cur, pb->schur_mu);
            pb->launches += 1;
        }
        if (pb->vinv_mu != mu) {
            launch_frame_inv(P, cur, mu, pb->stream);
            pb->vinv_mu = mu;
            pb->launches += 1;
        }
        launch_schur(P, cur, 1.0, pb->stream, 0, 0, nullptr, panels_ok(pb, cur, mu));
        panels_now(pb, cur, mu);
        pb->launches += 1;
    }
    pb->schur_mu = -1;
    if (pb->comm && !pb->s_reduced && !P.use_pcg) {
        StageTimer t(pb, &pb->times.allreduce);
        int rc = allreduce_system(pb, cur, 0);   // S (lower triangle) | rhs | g0
        if (rc) return rc;
    }
    pb->s_reduced = false;      // the factorisation below consumes the system
    pb->trial_reduced = false;
    if (P.use_spcg && !pb->force_direct && pb->spcg_skip > 0) pb->spcg_skip--;   // CG on the explicit reduced system instead of the LDL^T chain (S stays as it is)
    if (!chol_done) {
        StageTimer t(pb, &pb->times.chol);
        if (by_cg) launch_spcg(P, cur, mu, pb->stream);
        else launch_chol(P, cur, mu, pb->stream);
    }
    {
        StageTimer t(pb, &pb->times.backsub);
        launch_backsub(P, cur, tr, pb->stream);
    }
    pb->launches += 2 + 3 * P.nT;
    pb->blocks_valid = false;  // S of the current point has been eliminated in place
    if (evaluate_trial) {
        // predicted damping of the next step: every accepted step of the reference's rule with gain >= 0.94 gives 0.33 mu
        int rc = eval_blocks(pb, tr, mu * 0.33, cur, /*ents_ready=*/true);
        if (rc) return rc;
        pb->trial_points++;
    } else {
        HIP_TRY(hipMemsetAsync(P.err_part, 0, sizeof(double) * (size_t)std::max(n_err_terms(P), 1), pb->stream));
    }
    // The scalars go to the host BEFORE the speculative Schur complement of the trial point is queued: the host takes its
    // accept / reject decision and queues the next factorisation while that kernel runs, instead of after it.
    // On one GPU the reduction does not even get a launch of its own: it rides as one more workgroup of that kernel.
    int rc = AAR_OK;
    bool rode = false;
    if (P.use_pcg) {   // nothing is eliminated ahead of the next step in this mode: only the step's scalars travel
        if ((rc = launch_scalars(pb, n_err_terms(P)))) return rc;
    } else if (evaluate_trial && !pb->comm) {
        StageTimer t(pb, &pb->times.schur);
        rode = launch_schur(P, tr, 1.0, pb->stream, pb->seq + 1, n_err_terms(P), nullptr, panels_ok(pb, tr, mu * 0.33));
        panels_now(pb, tr, mu * 0.33);
        pb->launches += 1;
        if (rode) pb->seq++;
        else if ((rc = launch_scalars(pb, n_err_terms(P)))) return rc;   // (nothing rode: a rank without frames launches no Schur kernel)
    } else if (evaluate_trial && pb->fused_comm) {
        // Multi-GPU: this rank's scalars ride in the speculative Schur launch as on one GPU, but into the 8 doubles behind
        // g0 of the trial's block set, and ONE all-reduce then carries the step's scalars AND the next step's S | rhs | g0:
        // an accepted step with the predicted damping (the usual case) costs one collective, not two.
        {
            StageTimer t(pb, &pb->times.schur);
            rode = launch_schur(P, tr, 1.0, pb->stream, 0, n_err_terms(P), P.blk[tr].tail, panels_ok(pb, tr, mu * 0.33));
            panels_now(pb, tr, mu * 0.33);
            pb->launches += 1;
            if (!rode) { launch_reduce_scalars(P, n_err_terms(P), false, 0ull, pb->stream, P.blk[tr].tail); pb->launches += 1; }
        }
        pb->seq++;
        {
            StageTimer t(pb, &pb->times.allreduce);
            // tail[0..2] = sum r^2, sum |delta_f|^2, sum delta_f.g_f are rank sums, tail[3] carries every rank's error flags (so that
            // all ranks take the same branch); tail[5..6] (shared-parameter pieces) are computed from replicated data on every
            // rank and stay out of the reduction
            if ((rc = allreduce_system(pb, tr, 4, pb->seq))) return rc;   // (the unpacking kernel publishes the reduced scalars)
        }
        pb->trial_reduced = true;
        if (pb->spec_chol && !pb->stage_timers && !pb->profiling) {
            StageTimer t(pb, &pb->times.chol);
            // (the solver the NEXT try is expected to take: this try's own CG count is not known yet, the previous one's is)
            const bool spec_cg = P.use_spcg && pb->spcg_skip == 0 && !cg_near_cap;
            if (spec_cg) launch_spcg(P, tr, mu * 0.33, pb->stream);
            else launch_chol(P, tr, mu * 0.33, pb->stream);
            pb->spec_chol_by_cg = spec_cg;
            pb->spec_chol_blk = tr;
            pb->spec_chol_mu = mu * 0.33;
            pb->spec_chol_eta = P.pcg_eta_now;   // (a forcing SEQUENCE may switch to the tight term for the next try: that try then solves again)
            pb->launches += 3 * P.nT;
        }
    } else {
        if ((rc = launch_scalars(pb, n_err_terms(P)))) return rc;
        if (evaluate_trial) {
            StageTimer t(pb, &pb->times.schur);
            launch_schur(P, tr, 1.0, pb->stream, 0, 0, nullptr, panels_ok(pb, tr, mu * 0.33));
            panels_now(pb, tr, mu * 0.33);
            pb->launches += 1;
        }
    }
    if ((rc = check_async("kernel launch"))) return rc;
    if ((rc = wait_result(pb))) return rc;
    if (by_cg && pb->h_scal[7] >= 0.0) pb->last_cg_its = (int)pb->h_scal[7];
    // every rank must take the same decisions from last_cg_its, and the flags ARE joined over the ranks: a solve that gave up anywhere counts as one at the cap everywhere
    // (a time-out records SPCG_BUFS on the rank it happened on only)
    if (by_cg && (pb->h_flags[0] & (8 | 4))) pb->last_cg_its = std::min(P.spcg_max_it, SPCG_MAX_IT);
    if (cg_near_cap && P.use_spcg && !pb->force_direct && pb->spcg_skip == 0 && ++pb->near_cap_tries >= 8) { pb->last_cg_its = -1; pb->near_cap_tries = 0; }   // (the latch decays)
    if (pb->h_flags[0]) {
        (void)hipMemsetAsync(P.flags, 0, 4 * sizeof(int32_t), pb->stream);
        if (by_cg && (pb->h_flags[0] & (8 | 4))) {
            // the CG solve gave up (8: iteration cap; 4: a wavefront of its grid never showed up within ~1 s -- the device is shared): whatever
            // followed it in this try is meaningless, but S was not touched.  Not an error: the caller redoes the try with the direct chain.
            if (pb->h_flags[0] & 4) spcg_ws_reset(P, pb->stream);   // (a timed-out launch leaves slots of both buffer sets in an unknown state)
            pb->spcg_fallbacks++;
            pb->spcg_backoff = pb->spcg_backoff ? std::min(2 * pb->spcg_backoff, 1024) : 8;
            pb->spcg_skip = pb->spcg_backoff;
            return TRY_CG_FAILED;
        }
        set_error(AAR_ERR_NUMERIC, "device flags %d at mu=%g (1: a frame block is not positive definite, 2: non-positive pivot of the reduced system, 4: back-substitution chain timed out)", pb->h_flags[0], mu);
        // Only the reduced system lost positive definiteness (far from the optimum its Schur complement can, in floating point):
        // the LM loop takes that as a failed try and raises the damping; every rank sees the same replicated pivots.
        // (a zero or negative pivot fills the trial point with NaNs, which the next pass A reports as flag 1 as well: still a failed try)
        // (a back-substitution chain that timed out, flag 4, is never a failed try: its delta is garbage whatever the pivots were)
        return ((pb->h_flags[0] & 2) && !(pb->h_flags[0] & 4)) ? TRY_NOT_POSITIVE_DEFINITE : AAR_ERR_NUMERIC;
    }
    return AAR_OK;
}

// Rebuild the blocks of the current point after a rejected try consumed them (rare): everything the trial wrote into
// blk[1-cur] is garbage as well.
int rebuild_current(aar_problem *pb) {
    pb->mu_seed_valid = false;   // (the seed belongs to the blocks aar_lm_init built)
    int rc = zero_block_set(pb, pb->cur);
    if (rc) return rc;
    if ((rc = zero_block_set(pb, 1 - pb->cur))) return rc;
    // B = -J^T x64 of the reference is computed ONCE per step(), from the residual of the last accepted evaluation
    // (libs/sparselevmarq.h:367), i.e. with the Huber delta in force THEN -- the step callback may have moved it since
    const float huber_now = pb->P.huber;
    if (pb->with_huber && pb->huber_of_blocks > 0.f) pb->P.huber = pb->huber_of_blocks;
    rc = eval_blocks(pb, pb->cur, -1.0, -1);
    pb->P.huber = huber_now;
    if (rc) return rc;
    pb->blocks_valid = true;
    pb->vinv_mu = -1;
    pb->schur_mu = -1;
    pb->s_reduced = pb->trial_reduced = false;
    return AAR_OK;
}

// damped_try, and -- solver spcg -- the same try once more with the direct chain when the CG solve gave up (iteration cap, hand-over
// time-out): the blocks of the current point are rebuilt (the abandoned try's trial evaluation cleared them), the damping stays
int damped_try_fb(aar_problem *pb, double mu, bool evaluate_trial) {
    int rc = damped_try(pb, mu, evaluate_trial);
    if (rc != TRY_CG_FAILED) return rc;
    if (evaluate_trial) pb->trial_points--;   // (the abandoned try's trial evaluation is not a residual evaluation of the LM loop)
    pb->trial_reduced = false;
    if ((rc = rebuild_current(pb))) return rc;
    pb->force_direct = true;
    rc = damped_try(pb, mu, evaluate_trial);
    pb->force_direct = false;
    return rc;
}

// x_full -> z of the reference for the problem's Config (mats2eVec order: cameras | markers | frames), and back
void extract_z(const PoseLayout &L, const double *x_full, double *z) {
    int64_t k = 0;
    if (L.oc) for (int64_t i = 0; i < 6LL * (L.C - 1); i++) z[k++] = x_full[L.full_cam0() + i];
    if (L.om) for (int64_t i = 0; i < 6LL * (L.M - 1); i++) z[k++] = x_full[L.full_mk0() + i];
    if (L.of) for (int64_t i = 0; i < 6LL * L.F; i++) z[k++] = x_full[L.full_fr0() + i];
    if (L.oi) for (int64_t i = 0; i < 9LL * L.C; i++) z[k++] = x_full[L.full_intr0() + i];
}
void merge_z(const PoseLayout &L, const double *z, double *x_full) {
    int64_t k = 0;
    if (L.oc) for (int64_t i = 0; i < 6LL * (L.C - 1); i++) x_full[L.full_cam0() + i] = z[k++];
    if (L.om) for (int64_t i = 0; i < 6LL * (L.M - 1); i++) x_full[L.full_mk0() + i] = z[k++];
    if (L.of) for (int64_t i = 0; i < 6LL * L.F; i++) x_full[L.full_fr0() + i] = z[k++];
    if (L.oi) for (int64_t i = 0; i < 9LL * L.C; i++) x_full[L.full_intr0() + i] = z[k++];
}

// curr_z on the host for a callback (a device -> host copy per call: only made when a callback asked for it)
int current_z_for_callbacks(aar_problem *pb, const double *x_start) {
    pb->cb_x.assign(x_start, x_start + pb->L.full_len());
    int rc = download_z(pb, pb->cur, pb->cb_x.data());
    if (rc) return rc;
    pb->cb_z.resize((size_t)std::max<int64_t>(pb->L.z_len(), 1));
    extract_z(pb->L, pb->cb_x.data(), pb->cb_z.data());
    return AAR_OK;
}

int initial_mu(aar_problem *pb, double tau, double *mu) {
    DeviceProblem &P = pb->P;
    const int cur = pb->cur;
    if (pb->comm) {
        // the diagonal of the shared blocks is a sum over ranks; the frame blocks are rank-local
        HIP_TRY(hipMemcpy2DAsync(pb->d_diag, sizeof(double), P.blk[cur].S, (size_t)(P.n_pad + 1) * sizeof(double), sizeof(double),
                                 P.n_pad, hipMemcpyDeviceToDevice, pb->stream));
        int rc = allreduce(pb, pb->d_diag, P.n_pad, NCCL_SUM);
        if (rc) return rc;
        // the trial block set's S is zero and unused at this point: borrow its diagonal for the summed values
        HIP_TRY(hipMemcpy2DAsync(P.blk[1 - cur].S, (size_t)(P.n_pad + 1) * sizeof(double), pb->d_diag, sizeof(double), sizeof(double),
                                 P.n_pad, hipMemcpyDeviceToDevice, pb->stream));
        DeviceProblem Q = P;
        Q.blk[cur].S = P.blk[1 - cur].S;
        launch_maxdiag(Q, cur, pb->stream);
        HIP_TRY(hipMemsetAsync(P.blk[1 - cur].S, 0, (size_t)P.n_pad * P.n_pad * sizeof(double), pb->stream));
        rc = allreduce(pb, P.scal + 4, 1, NCCL_MAX);
        if (rc) return rc;
    } else {
        if (pb->schur_mu >= 0) {   // (the init head start has already reduced S for its damping: the diagonal of J^T J is read from the blocks, so give the terms back first)
            launch_schur(P, cur, -1.0, pb->stream, 0, 0, nullptr, panels_ok(pb, cur, pb->schur_mu));
            panels_now(pb, cur, pb->schur_mu);
            pb->schur_mu = -1;
            pb->launches += 1;
        }
        launch_maxdiag(P, cur, pb->stream);
    }
    pb->launches += 1;
    pb->seq++;
    launch_publish(P, pb->seq, pb->stream);
    int rc2 = wait_result(pb);
    if (rc2) return rc2;
    *mu = pb->h_scal[4] * tau;
    return AAR_OK;
}

}  // namespace

extern "C" {

int aar_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

int aar_device_synchronize(void) {
    HIP_TRY(hipDeviceSynchronize());
    return AAR_OK;
}

int aar_comm_make_id(char id[AAR_COMM_ID_BYTES]) {
    int rc = load_nccl();
    if (rc) return rc;
    NcclId u;
    NCCL_TRY(g_nccl.GetUniqueId(&u));
    memcpy(id, u.internal, AAR_COMM_ID_BYTES);
    return AAR_OK;
}

int aar_comm_create(const char id[AAR_COMM_ID_BYTES], int32_t world_size, int32_t rank, int32_t device_id, aar_comm **out) {
    if (!id || !out || world_size < 1 || rank < 0 || rank >= world_size) return set_error(AAR_ERR_INVALID, "aar_comm_create: bad arguments");
    int rc = load_nccl();
    if (rc) return rc;
    rc = ensure_device(device_id);
    if (rc) return rc;
    NcclId u;
    memcpy(u.internal, id, AAR_COMM_ID_BYTES);
    aar_comm *c = new aar_comm();
    c->world = world_size; c->rank = rank; c->device = device_id;
    int r = g_nccl.CommInitRank(&c->comm, world_size, u, rank);
    if (r != 0) {
        delete c;
        return set_error(AAR_ERR_COMM, "ncclCommInitRank failed: %s", g_nccl.GetErrorString ? g_nccl.GetErrorString(r) : "?");
    }
    *out = c;
    return AAR_OK;
}

int aar_comm_get_stats(const aar_comm *c, aar_comm_stats *out) {
    if (!c || !out) return set_error(AAR_ERR_INVALID, "aar_comm_get_stats: null argument");
    memset(out, 0, sizeof *out);
    out->world_size = c->world;
    out->rank = c->rank;
    out->ranks_seen = c->world;
    if (c->comm && g_nccl.CommCount) {   // what RCCL itself reports for this communicator
        int n = 0;
        NCCL_TRY(g_nccl.CommCount(c->comm, &n));
        out->ranks_seen = n;
    }
    out->allreduce_calls = c->allreduce_calls;
    out->allreduce_bytes = c->allreduce_bytes;
    out->system_allreduce_bytes = c->last_system_bytes;
    return AAR_OK;
}

void aar_comm_destroy(aar_comm *c) {
    if (!c) return;
    if (c->comm && g_nccl.ok) g_nccl.CommDestroy(c->comm);
    if (c->tmp) (void)hipFree(c->tmp);
    delete c;
}

int aar_local_group_create(int32_t world_size, aar_local_group **out) {
    if (!out || world_size < 1 || world_size > 64) return set_error(AAR_ERR_INVALID, "aar_local_group_create: bad arguments");
    aar_local_group *g = new aar_local_group();
    g->world = world_size;
    g->ptrs.assign(world_size, nullptr);
    *out = g;
    return AAR_OK;
}

void aar_local_group_destroy(aar_local_group *g) { delete g; }

int aar_comm_create_local(aar_local_group *group, int32_t rank, int32_t device_id, aar_comm **out) {
    if (!group || !out || rank < 0 || rank >= group->world) return set_error(AAR_ERR_INVALID, "aar_comm_create_local: bad arguments");
    int rc = ensure_device(device_id);
    if (rc) return rc;
    aar_comm *c = new aar_comm();
    c->world = group->world; c->rank = rank; c->device = device_id; c->local = group;
    *out = c;
    return AAR_OK;
}

void aar_lm_default_params(aar_lm_params *p) {  // libs/multicam_mapper.cpp:326-330 over libs/sparselevmarq.h:41-49
    p->max_iters = 10000;
    p->min_error = 1e-5;
    p->min_step_error_diff = 0;
    p->min_average_step_error_diff = 1e-4;
    p->tau = 1;
    p->verbose = 0;
}

void aar_problem_destroy(aar_problem *pb) {
    if (!pb) return;
    (void)hipSetDevice(pb->device);
    if (pb->stream) (void)hipStreamSynchronize(pb->stream);
    for (void *p : pb->allocs) (void)hipFree(p);
    if (pb->h_scal) (void)hipHostFree(pb->h_scal);
    if (pb->h_pcg) (void)hipHostFree(pb->h_pcg);
    if (pb->h_gather) (void)hipHostFree(pb->h_gather);
    if (pb->up_ev) (void)hipEventDestroy(pb->up_ev);
    if (pb->ev[0]) (void)hipEventDestroy(pb->ev[0]);
    if (pb->ev[1]) (void)hipEventDestroy(pb->ev[1]);
    for (hipEvent_t e : pb->ev_pool) (void)hipEventDestroy(e);
    if (pb->stream2) { (void)hipStreamSynchronize(pb->stream2); (void)hipStreamDestroy(pb->stream2); }
    if (pb->stream) (void)hipStreamDestroy(pb->stream);
    delete pb;
}

void aar_solver_default_options(aar_solver_options *o) {
    if (!o) return;
    memset(o, 0, sizeof *o);
    o->struct_size = (uint32_t)sizeof *o;
    o->solver = AAR_SOLVER_AUTO;
}

int aar_problem_create(const aar_problem_desc *d, aar_problem **out) { return aar_problem_create_ex(d, nullptr, out); }

// ---- constraints ----
static int problem_create(const aar_problem_desc *d, const aar_solver_options *opts, const aar_problem_constraints *cons, aar_problem **out);
namespace {
// the caller's struct at its own size; fields beyond it count as empty
aar_problem_constraints constraints_of(const aar_problem_constraints *c) {
    aar_problem_constraints k;
    memset(&k, 0, sizeof k);
    if (c) memcpy(&k, c, std::min<size_t>(c->struct_size, sizeof k));
    k.struct_size = (uint32_t)sizeof k;
    return k;
}
bool constraints_empty(const aar_problem_constraints &k) { return k.n_fixed_cams == 0 && k.n_fixed_markers == 0 && k.n_priors == 0 && k.n_pair_priors == 0; }
// symmetric positive semi-definite: LDL^T without pivoting, a negative pivot or a zero pivot over a non-zero column fails
bool info_psd(const double *I) {
    double scale = 0;
    for (int i = 0; i < 36; i++) scale = std::max(scale, std::fabs(I[i]));
    for (int i = 0; i < 6; i++)
        for (int j = 0; j < i; j++)
            if (std::fabs(I[6 * i + j] - I[6 * j + i]) > 1e-12 * scale) return false;
    if (scale == 0) return true;
    const double tol = 1e-13 * scale;
    double Lm[36] = {0}, D[6];
    for (int k = 0; k < 6; k++) {
        double d = I[6 * k + k];
        for (int j = 0; j < k; j++) d -= Lm[6 * k + j] * Lm[6 * k + j] * D[j];
        if (d < -tol) return false;
        for (int i = k + 1; i < 6; i++) {
            double v = I[6 * i + k];
            for (int j = 0; j < k; j++) v -= Lm[6 * i + j] * Lm[6 * k + j] * D[j];
            if (d <= tol) {
                if (std::fabs(v) > std::sqrt(tol * scale)) return false;
                Lm[6 * i + k] = 0;
            } else {
                Lm[6 * i + k] = v / d;
            }
        }
        D[k] = d <= tol ? 0.0 : d;
    }
    return true;
}
}  // namespace

int aar_problem_constraints_validate(const aar_problem_desc *d, const aar_problem_constraints *cons) {
    if (!d) return set_error(AAR_ERR_INVALID, "aar_problem_constraints_validate: null problem description");
    if (!cons) return AAR_OK;
    if (cons->struct_size < sizeof(uint32_t) + sizeof(int32_t)) return set_error(AAR_ERR_INVALID, "aar_problem_constraints.struct_size is not set");
    const aar_problem_constraints k = constraints_of(cons);
    const int C = d->num_cams, M = d->num_markers;
    if (k.n_fixed_cams < 0 || k.n_fixed_markers < 0 || k.n_priors < 0 || k.n_pair_priors < 0) return set_error(AAR_ERR_INVALID, "aar_problem_constraints: negative count");
    if ((k.n_fixed_cams && !k.fixed_cams) || (k.n_fixed_markers && !k.fixed_markers) || (k.n_priors && !k.priors) || (k.n_pair_priors && !k.pair_priors))
        return set_error(AAR_ERR_INVALID, "aar_problem_constraints: null array with a non-zero count");
    std::vector<uint8_t> fixed((size_t)std::max(C, 0) + std::max(M, 0), 0);
    for (int c = 0; c < C; c++) fixed[c] = (c == d->root_cam || !d->optimize_cam_poses) ? 1 : 0;
    for (int m = 0; m < M; m++) fixed[(size_t)C + m] = (m == d->root_marker || !d->optimize_marker_poses) ? 1 : 0;
    for (int i = 0; i < k.n_fixed_cams; i++) {
        const int c = k.fixed_cams[i];
        if (c < 0 || c >= C) return set_error(AAR_ERR_INVALID, "fixed_cams[%d] = %d: camera index out of range [0, %d)", i, c, C);
        fixed[c] = 1;
    }
    for (int i = 0; i < k.n_fixed_markers; i++) {
        const int m = k.fixed_markers[i];
        if (m < 0 || m >= M) return set_error(AAR_ERR_INVALID, "fixed_markers[%d] = %d: marker index out of range [0, %d)", i, m, M);
        fixed[(size_t)C + m] = 1;
    }
    std::vector<int32_t> owner(fixed.size(), -1);
    for (int p = 0; p < k.n_priors; p++) {
        const aar_pose_prior &q = k.priors[p];
        const char *what = q.kind == AAR_PRIOR_CAMERA ? "camera" : "marker";
        if (q.kind != AAR_PRIOR_CAMERA && q.kind != AAR_PRIOR_MARKER) return set_error(AAR_ERR_INVALID, "priors[%d]: kind %d is not AAR_PRIOR_CAMERA or AAR_PRIOR_MARKER", p, q.kind);
        const int lim = q.kind == AAR_PRIOR_CAMERA ? C : M;
        if (q.index < 0 || q.index >= lim) return set_error(AAR_ERR_INVALID, "priors[%d]: %s index %d out of range [0, %d)", p, what, q.index, lim);
        const size_t e = q.kind == AAR_PRIOR_CAMERA ? (size_t)q.index : (size_t)C + q.index;
        if (owner[e] >= 0) return set_error(AAR_ERR_INVALID, "priors[%d]: %s index %d already has a prior (priors[%d])", p, what, q.index, owner[e]);
        owner[e] = p;
        if (fixed[e]) return set_error(AAR_ERR_INVALID, "priors[%d]: %s index %d is fixed (root, non-optimised group or fixed index)", p, what, q.index);
        for (int i = 0; i < 6; i++)
            if (!std::isfinite(q.x6[i])) return set_error(AAR_ERR_INVALID, "priors[%d]: x6[%d] is not finite", p, i);
        for (int i = 0; i < 36; i++)
            if (!std::isfinite(q.info[i])) return set_error(AAR_ERR_INVALID, "priors[%d]: info[%d] is not finite", p, i);
        if (!info_psd(q.info)) return set_error(AAR_ERR_INVALID, "priors[%d]: the information matrix is not symmetric positive semi-definite (its Cholesky fails)", p);
    }
    std::map<std::pair<size_t, size_t>, int> seen;   // unordered pair of entities -> the entry that named it
    for (int p = 0; p < k.n_pair_priors; p++) {
        const aar_pair_prior &q = k.pair_priors[p];
        const char *what = q.kind == AAR_PRIOR_CAMERA ? "camera" : "marker";
        if (q.kind != AAR_PRIOR_CAMERA && q.kind != AAR_PRIOR_MARKER) return set_error(AAR_ERR_INVALID, "pair_priors[%d]: kind %d is not AAR_PRIOR_CAMERA or AAR_PRIOR_MARKER", p, q.kind);
        const int lim = q.kind == AAR_PRIOR_CAMERA ? C : M;
        if (q.index_a < 0 || q.index_a >= lim) return set_error(AAR_ERR_INVALID, "pair_priors[%d]: %s index_a %d out of range [0, %d)", p, what, q.index_a, lim);
        if (q.index_b < 0 || q.index_b >= lim) return set_error(AAR_ERR_INVALID, "pair_priors[%d]: %s index_b %d out of range [0, %d)", p, what, q.index_b, lim);
        if (q.index_a == q.index_b) return set_error(AAR_ERR_INVALID, "pair_priors[%d]: index_a and index_b are both %s %d", p, what, q.index_a);
        const size_t ea = q.kind == AAR_PRIOR_CAMERA ? (size_t)q.index_a : (size_t)C + q.index_a, eb = q.kind == AAR_PRIOR_CAMERA ? (size_t)q.index_b : (size_t)C + q.index_b;
        const auto ins = seen.insert({{std::min(ea, eb), std::max(ea, eb)}, p});
        if (!ins.second) return set_error(AAR_ERR_INVALID, "pair_priors[%d]: %ss %d and %d already have a pair prior (pair_priors[%d])", p, what, q.index_a, q.index_b, ins.first->second);
        if (fixed[ea] && fixed[eb])
            return set_error(AAR_ERR_INVALID, "pair_priors[%d]: %ss %d and %d are both fixed (root, non-optimised group or fixed index)", p, what, q.index_a, q.index_b);
        for (int i = 0; i < 6; i++)
            if (!std::isfinite(q.x6_rel[i])) return set_error(AAR_ERR_INVALID, "pair_priors[%d]: x6_rel[%d] is not finite", p, i);
        for (int i = 0; i < 36; i++)
            if (!std::isfinite(q.info[i])) return set_error(AAR_ERR_INVALID, "pair_priors[%d]: info[%d] is not finite", p, i);
        if (!info_psd(q.info)) return set_error(AAR_ERR_INVALID, "pair_priors[%d]: the information matrix is not symmetric positive semi-definite (its Cholesky fails)", p);
    }
    return AAR_OK;
}

int aar_problem_create_constrained(const aar_problem_desc *d, const aar_solver_options *opts, const aar_problem_constraints *cons, aar_problem **out) {
    if (!d || !out) return set_error(AAR_ERR_INVALID, "aar_problem_create_constrained: null argument");
    int rc = aar_problem_constraints_validate(d, cons);
    if (rc) return rc;
    if (!cons || constraints_empty(constraints_of(cons))) return aar_problem_create_ex(d, opts, out);
    const aar_problem_constraints k = constraints_of(cons);
    return problem_create(d, opts, &k, out);
}

int32_t aar_problem_num_priors(const aar_problem *pb) { return pb ? pb->P.n_prior : 0; }
int32_t aar_problem_num_pair_priors(const aar_problem *pb) { return pb ? pb->P.n_pair : 0; }

// AAR_ABORT_BACKTRACE=<file> (diagnostics): the native stack of whoever raises SIGABRT in this process (a runtime library giving up) is appended to the file before the default action
static int abort_bt_fd = 2;
static void abort_backtrace(int sig) {
    void *bt[64];
    { char msg[64]; const int k = aar::g_last_kernel_id; int n = 0; const char *t = "last kernel id "; while (t[n]) { msg[n] = t[n]; n++; } if (k < 0) msg[n++] = '-'; else { if (k >= 10) msg[n++] = '0' + k / 10; msg[n++] = '0' + k % 10; } msg[n++] = '\n'; (void)!write(abort_bt_fd, msg, n); }
    const int n = backtrace(bt, 64);
    backtrace_symbols_fd(bt, n, abort_bt_fd);
    signal(sig, SIG_DFL);
    raise(sig);
}

int aar_problem_create_ex(const aar_problem_desc *d, const aar_solver_options *opts, aar_problem **out) { return problem_create(d, opts, nullptr, out); }

// ------------------------------------------------------------------------------------------------
// Problem creation: a sequence of steps, each a function below; problem_create at the end calls them in order.  The index
// tables come from the planner (host/problem_plan.cpp): no step here builds one.
// ------------------------------------------------------------------------------------------------
namespace {

// Step 1's result: the caller's options with the environment's overrides, and every AAR_* variable of problem creation (an empty
// optional: the variable is not set -- the step that owns the default applies it where it always was applied)
struct CreateEnv {
    aar_solver_options so;
    int env_over = 0;                  // AAR_ENV_* bits
    DeviceProblem::Tuning tune;        // tuning switches of this problem (kernels.h, DeviceProblem::Tuning)
    PlanKnobs knobs;                   // the planner's part (its solver-dependent switches: choose_solver)
    bool stage_timers = false;
    std::optional<bool> merge_passes, fused_comm, spec_chol;
    std::optional<int> dense_from_passA, spcg_coarse, spcg_coarse_from, pcg_coarse, pcg_coarse_from, pcg_e_every, pcg_resident, spcg_spread;
    std::optional<double> pcg_eta_loose, pcg_abs_tol, pcg_eta_switch;
    std::optional<int> schur_mfma, schur_panel_mb, pcg_fused, pcg_w32, pcg_grid;
};

// ---- step 1: options struct and environment ----
int read_create_options(const aar_solver_options *opts, CreateEnv &E) {
    { static bool once = false; if (!once && getenv("AAR_ABORT_BACKTRACE")) { once = true; const int fd = open(getenv("AAR_ABORT_BACKTRACE"), O_WRONLY | O_CREAT | O_APPEND, 0644); if (fd >= 0) abort_bt_fd = fd; signal(SIGABRT, abort_backtrace); } }
    aar_solver_options &so = E.so;
    aar_solver_default_options(&so);
    if (opts) {   // a caller built against an older header passes a shorter struct: the fields it does not know keep their defaults
        if (opts->struct_size < 2 * sizeof(uint32_t)) return set_error(AAR_ERR_INVALID, "aar_solver_options.struct_size is not set (use aar_solver_default_options)");
        memcpy(&so, opts, std::min<size_t>(opts->struct_size, sizeof so));
        so.struct_size = (uint32_t)sizeof so;
    }
    // environment overrides (tuning / bisecting only: the options struct is the interface): they apply to fields the caller left at their defaults
    // -- an explicitly chosen solver, forcing term or cap always wins -- and are reported (aar_solver_stats.env_overrides)
    int &env_over = E.env_over;
    if (const char *e = getenv("AAR_SOLVER")) {
        if (so.solver == AAR_SOLVER_AUTO) {
            int v = -1;
            if (!strcmp(e, "direct")) v = AAR_SOLVER_DIRECT;
            else if (!strcmp(e, "pcg")) v = AAR_SOLVER_PCG;
            else if (!strcmp(e, "spcg")) v = AAR_SOLVER_SPCG;
            if (v >= 0) { so.solver = v; env_over |= AAR_ENV_SOLVER; }
        }
    }
    if (const char *e = getenv("AAR_DETERMINISTIC")) if (!so.deterministic && atoi(e) != 0) { so.deterministic = 1; env_over |= AAR_ENV_DETERMINISTIC; }
    if (const char *e = getenv("AAR_PCG_ETA")) if (so.pcg_eta == 0 && atof(e) > 0) { so.pcg_eta = atof(e); env_over |= AAR_ENV_PCG_ETA; }
    if (const char *e = getenv("AAR_PCG_MAX_IT")) if (so.pcg_max_it == 0 && atoi(e) > 0) { so.pcg_max_it = atoi(e); env_over |= AAR_ENV_PCG_MAX_IT; }
    if (so.solver < AAR_SOLVER_DIRECT || so.solver > AAR_SOLVER_AUTO) return set_error(AAR_ERR_INVALID, "aar_solver_options.solver %d is not one of AAR_SOLVER_*", so.solver);
    if (so.pcg_eta < 0 || so.pcg_max_it < 0 || so.pcg_eta_loose < 0 || so.pcg_eta_switch < 0 || so.pcg_abs_tol < 0) return set_error(AAR_ERR_INVALID, "aar_solver_options: negative pcg_eta / pcg_eta_loose / pcg_eta_switch / pcg_abs_tol / pcg_max_it");
    const char *tenv = getenv("AAR_STAGE_TIMERS");
    E.stage_timers = tenv && tenv[0] == '1';
    { const char *e = getenv("AAR_MERGE_PASSES"); if (e) E.merge_passes = (e[0] != '0'); }
    { const char *e = getenv("AAR_FUSED_COMM"); if (e) E.fused_comm = (e[0] != '0'); }
    { const char *e = getenv("AAR_SPEC_CHOL"); if (e) E.spec_chol = (e[0] != '0'); }
    {   // tuning switches of this problem (kernels.h, DeviceProblem::Tuning)
        auto env_int = [](const char *name, int &v) { if (const char *e = getenv(name)) v = atoi(e); };
        env_int("AAR_FUSED_PANEL", E.tune.fused_panel); env_int("AAR_BS_RIDES", E.tune.bs_rides);
        env_int("AAR_LDL_LOOKAHEAD", E.tune.lookahead); env_int("AAR_PASSA_VARIANT", E.tune.passA_variant); env_int("AAR_PACK_SYSTEM", E.tune.pack_system);
        env_int("AAR_INIT_HEADSTART", E.tune.init_headstart); env_int("AAR_PASSA_WRENCH", E.tune.passA_wrench); env_int("AAR_PASSAB_OCC2", E.tune.passAB_occ2);
    }
    { const char *e = getenv("AAR_DENSE_FROM_PASSA"); if (e) E.dense_from_passA = atoi(e) != 0 ? 1 : 0; }
    if (const char *t = getenv("AAR_SPCG_COARSE")) E.spcg_coarse = atoi(t) != 0;
    if (const char *t = getenv("AAR_SPCG_COARSE_FROM")) E.spcg_coarse_from = atoi(t);
    if (const char *t = getenv("AAR_PCG_COARSE")) E.pcg_coarse = atoi(t) != 0;
    if (const char *t = getenv("AAR_PCG_COARSE_FROM")) E.pcg_coarse_from = atoi(t);
    if (const char *t = getenv("AAR_PCG_E_EVERY")) E.pcg_e_every = std::max(1, atoi(t));
    if (const char *t = getenv("AAR_PCG_RESIDENT")) E.pcg_resident = atoi(t) != 0;
    if (const char *t = getenv("AAR_SPCG_SPREAD")) E.spcg_spread = std::max(1, atoi(t));
    if (const char *e = getenv("AAR_PCG_ETA_LOOSE")) E.pcg_eta_loose = atof(e);
    if (const char *e = getenv("AAR_PCG_ABS_TOL")) E.pcg_abs_tol = atof(e);
    if (const char *e = getenv("AAR_PCG_ETA_SWITCH")) E.pcg_eta_switch = atof(e);
    if (const char *e = getenv("AAR_SCHUR_MFMA")) E.schur_mfma = atoi(e);
    if (const char *e = getenv("AAR_SCHUR_PANEL_MB")) E.schur_panel_mb = atoi(e);
    if (const char *t = getenv("AAR_PCG_FUSED")) E.pcg_fused = atoi(t) != 0 ? 1 : 0;
    if (const char *t = getenv("AAR_PCG_W32")) E.pcg_w32 = atoi(t) != 0 ? 1 : 0;
    if (const char *t = getenv("AAR_PCG_GRID")) E.pcg_grid = std::max(1, atoi(t));
    // the planner's knobs (host/problem_plan.h)
    if (const char *e = getenv("AAR_PASSB_CHUNK")) E.knobs.passb_chunk = atoi(e);
    if (const char *e = getenv("AAR_SCHUR_ITEM")) E.knobs.schur_item = atoi(e);
    if (const char *e = getenv("AAR_SCHUR_WINDOW")) E.knobs.schur_window = atoi(e);
    if (const char *e = getenv("AAR_SCHUR_XCD")) E.knobs.schur_xcd = atoi(e);
    if (const char *e = getenv("AAR_SCHUR_SPLIT")) E.knobs.schur_split = atoi(e);
    if (const char *t = getenv("AAR_PCG_CHUNK")) E.knobs.pcg_chunk = atoll(t);
    return AAR_OK;
}

// ---- step 2: validation and counting ----
int validate_and_count(const aar_problem_desc *d, std::vector<int64_t> &per_frame, int64_t &global_slots) {
    const int C = d->num_cams, M = d->num_markers, Fg = d->num_frames;
    const int64_t Ng = d->num_obs;
    if (C < 1 || M < 1 || Fg < 0 || Ng < 0) return set_error(AAR_ERR_INVALID, "aar_problem_create: bad sizes");
    if (d->root_cam < 0 || d->root_cam >= C || d->root_marker < 0 || d->root_marker >= M)
        return set_error(AAR_ERR_INVALID, "aar_problem_create: root index out of range");
    if (!d->cam_mats || (Ng > 0 && (!d->obs_frame || !d->obs_cam || !d->obs_marker || !d->obs_uv)))
        return set_error(AAR_ERR_INVALID, "aar_problem_create: null array");
    if (Ng >= (1LL << 31) || (int64_t)C + M >= 32768) return set_error(AAR_ERR_UNSUPPORTED, "problem too large for 32-bit indexing");
    per_frame.assign(Fg, 0);
    // (entity, frame) incidences of the WHOLE data set, counted the same way on every rank: what AUTO's choice between the two CG solvers rests on must not
    // depend on which frames a rank happens to own (ranks that chose differently would wait in different collectives forever)
    global_slots = 0;
    std::vector<int32_t> seen_c(C, -1), seen_m(M, -1);
    for (int64_t o = 0; o < Ng; o++) {
        const int f = d->obs_frame[o], c = d->obs_cam[o], m = d->obs_marker[o];
        if (f < 0 || f >= Fg || c < 0 || c >= C || m < 0 || m >= M) return set_error(AAR_ERR_INVALID, "observation %lld has an index out of range", (long long)o);
        if (o > 0 && f < d->obs_frame[o - 1]) return set_error(AAR_ERR_INVALID, "observations must be ordered by frame (reference residual order)");
        per_frame[f]++;
        if (seen_c[c] != f) { seen_c[c] = f; global_slots += d->optimize_cam_intrinsics ? 2 : 1; }
        if (seen_m[m] != f) { seen_m[m] = f; global_slots += 1; }
    }
    return AAR_OK;
}

// ---- step 3: device, streams and events (pb: freshly made, its device selected) ----
int open_streams(const aar_problem_desc *d, const CreateEnv &E, aar_problem *pb) {
    pb->device = d->device_id;
    pb->comm = d->comm;
    aar_lm_default_params(&pb->prm);
    memset(&pb->times, 0, sizeof pb->times);
    pb->stage_timers = E.stage_timers;
    if (hipStreamCreateWithFlags(&pb->stream, hipStreamNonBlocking) != hipSuccess) return set_error(AAR_ERR_HIP, "hipStreamCreate failed");
    (void)hipEventCreate(&pb->ev[0]);
    (void)hipEventCreate(&pb->ev[1]);
    if (hipStreamCreateWithFlags(&pb->stream2, hipStreamNonBlocking) != hipSuccess)
        return set_error(AAR_ERR_HIP, "second stream could not be created");
    if (E.merge_passes) pb->merge_passes = *E.merge_passes;
    if (E.fused_comm) pb->fused_comm = *E.fused_comm;
    if (E.spec_chol) pb->spec_chol = *E.spec_chol;
    return AAR_OK;
}

// ---- step 4: layout, shard by frame range, sizes ----
int plan_shard(const aar_problem_desc *d, const std::vector<int64_t> &per_frame, aar_problem *pb) {
    const int C = d->num_cams, M = d->num_markers, Fg = d->num_frames;
    PoseLayout &L = pb->L;
    L.C = C; L.M = M; L.F = Fg; L.rc = d->root_cam; L.rm = d->root_marker;
    L.oc = d->optimize_cam_poses != 0; L.om = d->optimize_marker_poses != 0; L.of = d->optimize_object_poses != 0;
    L.oi = d->optimize_cam_intrinsics != 0;
    pb->N_global = d->num_obs;

    const int world = pb->comm ? pb->comm->world : 1, rank = pb->comm ? pb->comm->rank : 0;
    pb->P.pcg_rank0 = rank == 0 ? 1 : 0;
    std::vector<int32_t> begin(world + 1, 0);
    int rc;
    if ((rc = aar_plan_shards(Fg, per_frame.data(), world, begin.data()))) return rc;
    pb->f_begin = begin[rank];
    pb->f_end = begin[rank + 1];
    int64_t ob = 0;
    for (int f = 0; f < pb->f_begin; f++) ob += per_frame[f];
    int64_t N = 0;
    for (int f = pb->f_begin; f < pb->f_end; f++) N += per_frame[f];
    pb->o_begin = ob;

    DeviceProblem &P = pb->P;
    // optimize_cam_intrinsics: one more shared entity per camera (fx, cx, fy, cy and two idle slots), after cameras and markers
    P.intr = L.oi ? 1 : 0;
    P.C = C; P.M = M; P.A = C + M + (L.oi ? C : 0); P.F = pb->f_end - pb->f_begin; P.N = N;
    P.n = 6 * P.A;
    P.nT = (P.n + CHOL_NB - 1) / CHOL_NB;
    P.n_pad = P.nT * CHOL_NB;
    // solver spcg, coarse space (spcg_kernels.hip, k_spcg_pre): a group with free entities lends its root's slot to the group's rigid-motion unknowns
    P.spcg_root_c = (L.oc && C > 1) ? L.rc : -1;
    P.spcg_root_m = (L.om && M > 1) ? C + L.rm : -1;
    P.spcg_n_free = (L.oc ? C - 1 : 0) + (L.om ? M - 1 : 0) + (L.oi ? C : 0);
    P.res_f32 = d->residual_mode == AAR_RES_F64 ? 0 : 1;
    pb->with_huber = d->with_huber != 0;
    P.huber = pb->with_huber ? pb->hubber_delta : -1.f;
    P.half_size = (double)((float)d->marker_size / 2.f);
    P.frames_fixed = L.of ? 0 : 1;
    return AAR_OK;
}

// ---- step 6: solver choice and limits.  global_slots: (entity, frame) incidences of the whole data set; held_extra: the caller fixed entities that
// would be free otherwise; local_rc: this rank's status so far (the first limit that is exceeded is kept); schur_mfma: which Schur kernel ----
void choose_solver(aar_problem *pb, const CreateEnv &E, int64_t global_slots, bool held_extra, int &local_rc, bool &schur_mfma) {
    DeviceProblem &P = pb->P;
    const PoseLayout &L = pb->L;
    const aar_solver_options &so = E.so;
    const int A = P.A, F = P.F, Fg = L.F, world = pb->comm ? pb->comm->world : 1;
    P.tune = E.tune;
    // the frame-block kernel keeps a frame's slots in LDS: sized by the form that is actually launched (wrench form: 21 + 4 doubles per slot; row form: 62)
    const size_t ldsA = P.tune.passA_wrench ? passA_wrench_lds_bytes(P.max_kf, L.oi)
                                            : std::max(passA_lds_bytes(P.max_kf, 256), passA_lds_bytes(P.max_kf, 64));
    if (ldsA > 160 * 1024 && !local_rc) local_rc = set_error(AAR_ERR_UNSUPPORTED, "a frame touches %d cameras+markers: %zu bytes of LDS in the frame-block kernel (%s form), the CU has 160 KiB", P.max_kf, ldsA, P.tune.passA_wrench ? "wrench" : "row");
    // Which Schur kernel (solve_kernels.hip): the MFMA kernel works on dense per-frame panels and is the default from 96 shared
    // entities, where the output-stationary kernel's re-reads of W dominate (config 5); AAR_SCHUR_MFMA=0 / 1 forces it (tests
    // force it on small problems).  Its panels cost 2 F Ad 288 bytes -- tens of GB for long sequences with many rarely seen
    // entities -- so they must fit a budget (half of the free device memory; AAR_SCHUR_PANEL_MB overrides), else the
    // output-stationary kernel, which needs none of this, takes over.  Only THAT kernel keeps a row panel of all entities in LDS.
    P.deterministic = so.deterministic ? 1 : 0;
    if (E.dense_from_passA) P.dense_from_passA = *E.dense_from_passA;
    {   // which solver (aar_solver_options; AUTO: DESIGN.md section 12)
        hipDeviceProp_t prop;
        const int cus = (hipGetDeviceProperties(&prop, pb->device) == hipSuccess && prop.multiProcessorCount > 0) ? prop.multiProcessorCount : 64;
        P.n_cus = cus;
        const bool pcg_ok = pcg_lds_bytes(A) <= 150 * 1024;
        // one wavefront per entity, every one of them resident AT ONCE (they hand over to each other): asked of the runtime's occupancy calculator for this
        // kernel's registers and LDS, as pcg_max_grid asks for the PCG grid.  (Another process on the device can still take the slots: k_spcg's time-out.)
        if (E.spcg_coarse) P.spcg_coarse = *E.spcg_coarse;
        if (E.spcg_coarse_from) P.spcg_coarse_from = *E.spcg_coarse_from;
        if (E.pcg_coarse) P.pcg_coarse = *E.pcg_coarse;
        if (E.pcg_coarse_from) P.pcg_coarse_from = *E.pcg_coarse_from;
        // both coarse spaces are built for groups whose only fixed entity is the root (its slot carries the group's rigid motion): with entities
        // fixed by the caller they are off
        if (held_extra) { P.spcg_coarse = 0; P.pcg_coarse = 0; }
        // the coarse operator's pass costs like ~1.5 CG iterations and a kept operator ~0.1 - 0.7 more iterations per solve: keeping it pays on long sequences only
        // (profiles/r06_attempts.txt section 3: +3.7 % at 160 entities x 4 000 frames, +1.4 % at config 5, -1 .. -3 % on 500-frame problems)
        P.pcg_e_every = P.total_slots >= 300000 ? 3 : 1;
        if (E.pcg_e_every) P.pcg_e_every = *E.pcg_e_every;
        if (E.pcg_resident) P.pcg_resident = *E.pcg_resident;
        if (pcg_lds_bytes(A, true) > 150 * 1024) P.pcg_coarse = 0;   // (the coarse space's tables do not fit beside the vectors of this many entities: block-Jacobi only)
        const int spcg_per_cu = spcg_fits(P.nT) ? spcg_resident_per_cu(P.nT, spcg_coarse_now(P)) : 0;
        const bool spcg_ok = spcg_fits(P.nT) && P.n_pad / 6 <= std::max(1, spcg_per_cu) * cus;
        int solver = so.solver;
        if (solver == AAR_SOLVER_AUTO) {
            // Measured on MI355X at the default forcing terms (profiles/r05_auto_crossover.txt; scripts/dev/auto_crossover.py):
            //  * one tile of unknowns (up to 16 cameras + markers): the direct chain is a single 25-us launch -- about what 10 CG iterations cost;
            //  * CG on the EXPLICIT Schur complement (SPCG) beats both the LDL^T chain and the CG through the frame blocks wherever it fits (up to 224 shared
            //    entities), 48 .. 216 entities x 500 frames: 1.6x .. 1.4x the direct chain, 3.2x .. 1.1x PCG;
            //  * PCG never forms the complement: its step costs (CG iterations) x (a pass over the frames' W blocks -- fp32 since round 5), SPCG's one Schur complement
            //    (work ~ slots x slots-per-frame) + CG iterations of ~1.7 us.  PCG overtakes on long sequences of frames that each see many entities: measured
            //    crossovers (PCG with fp32 blocks and the barrier tree) at ~45 k (entity, frame) incidences for 122 per frame (216 entities), ~85 k for 92 (160
            //    entities), ~95 k for 64 (112 entities) -- fitted by  incidences x (incidences per frame - 30) >= 4e6.
            // The rule is applied to a rank's SHARE of the whole data set (shards are balanced by observation count), from numbers every rank holds.
            const double kf_avg = Fg > 0 ? (double)global_slots / (double)Fg : 0.0;
            const bool pcg_pays = A >= 96 && pcg_ok && (double)global_slots / (double)world * (kf_avg - 30.0) >= 4e6;
            if (P.nT < 2) solver = AAR_SOLVER_DIRECT;
            else if (spcg_ok && !pcg_pays) solver = AAR_SOLVER_SPCG;
            else if (pcg_ok) solver = AAR_SOLVER_PCG;
            else solver = AAR_SOLVER_DIRECT;
        }
        pb->solver = solver;
        pb->env_overrides = E.env_over;
        P.use_pcg = solver == AAR_SOLVER_PCG ? 1 : 0;
        P.use_spcg = solver == AAR_SOLVER_SPCG ? 1 : 0;
        if (E.spcg_spread) P.spcg_spread = *E.spcg_spread;
        // (one XCD has an eighth of the CUs: more entities than that many wavefront slots would not all be resident there)
        if (P.n_pad / 6 > std::min(4, std::max(1, spcg_per_cu)) * (cus / 8)) P.spcg_spread = 1;
        // Forcing term of the inexact solvers (include/aar.h; defaults and why: kernels.h).  The CG through the frame blocks measures |r| / |b|; the CG on the
        // explicit system measures in the preconditioner's norm (r^T M^-1 r, which its recurrences carry anyway).  pcg_eta_loose > pcg_eta: a forcing sequence (opt-in).
        P.pcg_eta = P.use_spcg ? SPCG_ETA_DEFAULT : PCG_ETA_DEFAULT;
        if (so.pcg_eta > 0) P.pcg_eta = so.pcg_eta;
        P.pcg_eta_loose = 0.0;
        if (so.pcg_eta_loose > 0) P.pcg_eta_loose = so.pcg_eta_loose;
        else if (so.pcg_eta == 0 && (P.use_pcg || P.use_spcg)) P.pcg_eta_loose = P.use_pcg ? PCG_ETA_LOOSE_DEFAULT : SPCG_ETA_LOOSE_DEFAULT;   // (0: none)
        if (E.pcg_eta_loose) if (so.pcg_eta_loose == 0) P.pcg_eta_loose = *E.pcg_eta_loose;
        if (P.pcg_eta_loose <= P.pcg_eta) P.pcg_eta_loose = 0.0;   // (no sequence: one forcing term throughout)
        P.pcg_abs_tol = P.use_pcg ? PCG_ABS_TOL_DEFAULT : SPCG_ABS_TOL_DEFAULT;
        if (so.pcg_abs_tol > 0) P.pcg_abs_tol = so.pcg_abs_tol;
        else if (E.pcg_abs_tol) P.pcg_abs_tol = *E.pcg_abs_tol;
        if (so.pcg_eta_switch > 0) P.pcg_eta_switch = so.pcg_eta_switch;
        else if (E.pcg_eta_switch) P.pcg_eta_switch = *E.pcg_eta_switch;
        P.pcg_eta_now = P.pcg_eta;
        P.spcg_max_it = spcg_default_cap(P.nT);
        if (so.pcg_max_it > 0) { P.pcg_max_it = so.pcg_max_it; P.spcg_max_it = std::min(so.pcg_max_it, SPCG_MAX_IT); }
        if (P.use_pcg && !pcg_ok && !local_rc) local_rc = set_error(AAR_ERR_UNSUPPORTED, "AAR_SOLVER_PCG keeps the CG vectors and the preconditioner of %d unknowns in LDS: too many shared entities", 6 * A);
        if (P.use_spcg && !spcg_ok && !local_rc) local_rc = set_error(AAR_ERR_UNSUPPORTED, "AAR_SOLVER_SPCG keeps the reduced system in the registers of one wavefront per shared entity: %d unknowns are too many (limit %d, and at most %d entities)", 6 * A, 96 * SPCG_MAX_NT, std::max(1, spcg_per_cu) * cus);
    }
    schur_mfma = A >= 96 && F > 0;
    if (E.schur_mfma) schur_mfma = *E.schur_mfma != 0 && F > 0;
    if (P.deterministic) schur_mfma = false;   // fixed-order sums exist for the output-stationary kernel only (kernels.h)
    if (P.use_pcg) schur_mfma = true;          // (no Schur complement is ever formed in that mode: no LDS row panel to fit; the dense panels are not allocated either)
    if (schur_mfma) {
        const size_t panel_bytes = (size_t)2 * F * ((A + 1 + 31) / 32 * 32) * 288;
        size_t free_b = 0, total_b = 0;
        size_t budget = (hipMemGetInfo(&free_b, &total_b) == hipSuccess) ? free_b / 2 : (size_t)64 << 30;
        if (E.schur_panel_mb) budget = (size_t)std::max(0, *E.schur_panel_mb) << 20;
        if (panel_bytes > budget) schur_mfma = false;
    }
    if (!schur_mfma && (size_t)A * 36 * 8 + 2048 > 160 * 1024 && !local_rc)
        local_rc = set_error(AAR_ERR_UNSUPPORTED, "%d cameras+markers exceed the row panel the output-stationary Schur kernel holds in LDS (and the dense panels of the MFMA kernel do not fit the memory budget)", A);
}

// ---- step 7: collective agreement.  The limits above depend on the rank's own frames: agree on the outcome before anybody returns (see collective_status) ----
int agree_on_status(aar_problem *pb, int local_rc) {
    int rc;
    if (pb->comm && (rc = dev_alloc(pb, &pb->d_status, 1))) return rc;
    int agreed = local_rc;
    if ((rc = collective_status(pb, local_rc, &agreed))) return rc;
    if (local_rc) return local_rc;
    if (agreed) return set_error(agreed, "another rank could not create its shard of the problem (status %d)", agreed);
    return AAR_OK;
}

// the device reads the planner's pair_rec as int4
static_assert(sizeof(PairRec) == sizeof(int4) && alignof(int4) % alignof(PairRec) == 0 && offsetof(PairRec, frame) == 0 && offsetof(PairRec, slot) == 4 &&
              offsetof(PairRec, frame_slot0) == 8 && offsetof(PairRec, pad) == 12, "PairRec must lay out as the int4 {x, y, z, w} the kernels read");

// ---- step 9: upload of the plan's tables (and the counts that go with them) ----
int upload_plan(aar_problem *pb, const aar_problem_desc *d, const FramePlan &fp, const TablePlan &tp) {
    DeviceProblem &P = pb->P;
    int rc;
    P.n_chunks = tp.n_chunks; P.n_swork = tp.n_swork;
    P.n_pbr = tp.n_pbr; P.pb_stride = tp.pb_stride;
    P.Ad = tp.Ad; P.n_smwork = tp.n_smwork;
    P.pcg_n_items = tp.pcg_n_items;
    spcg_build_fixed_mask(P, tp.ent_fixed.data());   // (k_spcg reads the same flags as bits in its arguments)
    std::vector<double> Kh(d->cam_mats, d->cam_mats + 9 * (size_t)P.C);
#define UP(field, vec) if ((rc = dev_upload(pb, &P.field, vec))) return rc
    UP(K, Kh); UP(a_idx, fp.a_idx); UP(a_uv, fp.a_uv); UP(frame_obs_start, fp.frame_obs_start); UP(frame_stride, fp.frame_stride);
    UP(fslot_start, fp.fslot_start); UP(fslot_ent, fp.fslot_ent); UP(b_idx, tp.b_idx); UP(b_uv, tp.b_uv);
    UP(chunk_start, tp.chunk_start); UP(ent_fixed, tp.ent_fixed); UP(up_start, tp.up_start); UP(up_ent, tp.up_ent);
    UP(sw_ent, tp.sw_ent); UP(sw_begin, tp.sw_begin); UP(sw_end, tp.sw_end);
    if ((rc = dev_upload(pb, reinterpret_cast<PairRec **>(&P.pair_rec), tp.pair_rec))) return rc;
    if (P.use_pcg) { UP(pcg_it_ent, tp.pcg_it_ent); UP(pcg_it_begin, tp.pcg_it_begin); UP(pcg_it_end, tp.pcg_it_end); UP(pcg_ent_item_start, tp.pcg_ent_item_start); }
    if (P.deterministic) { UP(sp_off, tp.sp_off); UP(se_start, tp.se_start); UP(se_items, tp.se_items); UP(pbr_start, tp.pbr_start); UP(pbr_chunk, tp.pbr_chunk); UP(pbr_kind, tp.pbr_kind); UP(pbr_a, tp.pbr_a); UP(pbr_b, tp.pbr_b); }
    if (P.n_smwork) { UP(sm_ga, tp.sm_ga); UP(sm_gb, tp.sm_gb); UP(sm_fb, tp.sm_fb); UP(sm_fe, tp.sm_fe); UP(slot_dense, tp.slot_dense); UP(slot_frame, tp.slot_frame); UP(dense_ent, tp.dense_ent); UP(sm_frames, tp.sm_frames); }
#undef UP
    return AAR_OK;
}

#define AL(field, count) if ((rc = dev_alloc(pb, &P.field, (size_t)(count)))) return rc

// ---- step 10: workspaces ----
int alloc_workspaces(aar_problem *pb, const CreateEnv &E, int64_t sp_total) {
    DeviceProblem &P = pb->P;
    const int A = P.A, F = P.F;
    const int64_t N = P.N;
    int rc;
    AL(z[0], 6 * (size_t)(A + F)); AL(z[1], 6 * (size_t)(A + F));
    AL(ent[0], (size_t)(A + F) * ENT_STRIDE); AL(ent[1], (size_t)(A + F) * ENT_STRIDE);
    for (int w = 0; w < 2; w++) {
        AL(blk[w].V, (size_t)F * 36); AL(blk[w].gf, (size_t)F * 6); AL(blk[w].W, (size_t)P.total_slots * 36);
        AL(blk[w].Vinv, (size_t)F * 36); AL(blk[w].hf, (size_t)F * 6);
        // rhs and g0 live right behind S: ONE all-reduce makes all three global on the multi-GPU path (g0, the shared part of
        // B = -J^T r, is added to the right-hand side on first touch and enters delta.B, so every rank needs all of it)
        AL(blk[w].S, (size_t)P.n_pad * P.n_pad + 2 * (size_t)P.n_pad + 8);
        P.blk[w].rhs = P.blk[w].S + (size_t)P.n_pad * P.n_pad;
        P.blk[w].g0 = P.blk[w].rhs + P.n_pad;
        P.blk[w].tail = P.blk[w].g0 + P.n_pad;
        if (hipMemset(P.blk[w].tail, 0, 8 * sizeof(double)) != hipSuccess) return set_error(AAR_ERR_HIP, "hipMemset failed");
    }
    if (P.deterministic) { AL(sp_part, (size_t)sp_total); AL(pb_part, (size_t)P.n_chunks * P.pb_stride); }
    if (P.use_pcg) {
        AL(pcg_ws, (size_t)P.pcg_n_items * 28 + 6 * (size_t)F + 8); AL(pcg_counter, 8);
        AL(pcg_yg, (size_t)3 * PCG_NYV * P.n_pad + (size_t)28 * A + 160 + 8); AL(pcg_hop, 2 * PCG_HOP_WORDS);   // (+ 160: the coarse operator's accumulator)
        if (E.pcg_fused) P.pcg_fused = *E.pcg_fused;
        {   // k_pcgf's operator reads an fp32 copy of W (half the bytes of its pass over the frames; written by pass A instead of the fp64 blocks): non-deterministic runs, one rank or many
            int w32 = 1;
            if (E.pcg_w32) w32 = *E.pcg_w32;
            if (w32 && P.pcg_fused && !P.deterministic && P.pcg_eta >= PCG_W32_MIN_ETA)   // (a caller who asks for residuals below 1e-4 gets fp64 blocks throughout)
                for (int w = 0; w < 2; w++) AL(blk[w].Wf, (size_t)P.total_slots * 36 + 4);
        }
        P.pcg_grid = P.n_cus;   // one workgroup per CU: all resident
        // small problems: fewer workgroups make the two grid-wide hand-overs of an iteration cheaper than the passes get slower
        // (measured, LM it/s at config 3: 64 / 128 / 256 workgroups 4174 / 4201 / 3883; config 2: 32 best; config 5: 256 best)
        const int64_t want = std::max<int64_t>(32, ((int64_t)F + 3) / 4);
        P.pcg_grid = (int)std::min<int64_t>(P.pcg_grid, want);
        if (pb->comm) {
            AL(pcgd_setup, (size_t)A * 28 + 152); AL(pcgd_minv, (size_t)A * 36 + 72 + (size_t)12 * A + 8);   // (+ the coarse operator's shares; + its inverse blocks and the table of Z)
            AL(pcgd_state, 2 * (18 * (size_t)A + 8)); AL(pcgd_y, 3 * (6 * (size_t)A + 8));
            if (hipHostMalloc((void **)&pb->h_pcg, 8 * sizeof(double), hipHostMallocMapped | hipHostMallocCoherent) != hipSuccess)
                return set_error(AAR_ERR_HIP, "hipHostMalloc failed");
            memset(pb->h_pcg, 0, 8 * sizeof(double));
            if (hipHostGetDevicePointer((void **)&P.pcgd_host, pb->h_pcg, 0) != hipSuccess) return set_error(AAR_ERR_HIP, "hipHostGetDevicePointer failed");
        }
        if (E.pcg_grid) P.pcg_grid = *E.pcg_grid;
        // the kernels' grid-wide hand-overs need every workgroup resident: never more than the occupancy query admits (the override included),
        // asked at the footprint they are launched with (P.pcg_coarse is final: cut above where its tables do not fit)
        P.pcg_grid = std::min(P.pcg_grid, pcg_max_grid(A, P.pcg_coarse != 0, P.n_cus));
    }
    if (P.use_spcg) {
        AL(spcg_ws, spcg_ws_doubles(P.n_pad)); AL(spcg_iters, 8);
        if (spcg_coarse_now(P)) AL(spcg_pre, spcg_pre_doubles(P.n_pad));   // (zeroed: the restriction rows' columns of fixed entities stay zero)
        spcg_ws_reset(P, pb->stream);
    }
    if (P.n_smwork) { AL(Wd, (size_t)F * P.Ad * 36); AL(Yd, (size_t)F * P.Ad * 36); }   // zeroed here, once: absent pairs are never written
    AL(Dfac, (size_t)P.nT * CHOL_NB * CHOL_NB); AL(Linv16, (size_t)P.nT * (CHOL_NB / 16) * 256); AL(delta_s, P.n_pad); AL(bs_flags, (size_t)P.nT);
    AL(Lp, (size_t)P.nT * P.n_pad * CHOL_NB); AL(zf, P.n_pad);
    AL(err_part, std::max<size_t>((size_t)F, (size_t)((N + 255) / 256)) + 1);
    AL(lin_part, 2 * (size_t)(F + 1)); AL(scal, 8); AL(flags, 4);
    return AAR_OK;
}

// ---- step 11: priors (the pose priors' and pair priors' data, the pair priors' element lists from the plan, their outputs) ----
int upload_priors(aar_problem *pb, const aar_problem_constraints *cons, const TablePlan &tp) {
    DeviceProblem &P = pb->P;
    const int C = P.C, rank = pb->comm ? pb->comm->rank : 0;
    int rc;
    if (cons && cons->n_priors > 0) {
        const int np_ = cons->n_priors;
        std::vector<int32_t> pent(np_);
        std::vector<double> pdat((size_t)np_ * PRIOR_DAT);
        for (int p = 0; p < np_; p++) {
            const aar_pose_prior &q = cons->priors[p];
            pent[p] = q.kind == AAR_PRIOR_CAMERA ? q.index : C + q.index;
            memcpy(&pdat[(size_t)p * PRIOR_DAT], q.x6, 6 * sizeof(double));
            memcpy(&pdat[(size_t)p * PRIOR_DAT + 6], q.info, 36 * sizeof(double));
        }
        if ((rc = dev_upload(pb, &P.prior_ent, pent)) || (rc = dev_upload(pb, &P.prior_dat, pdat))) return rc;
        AL(prior_out, (size_t)np_ * 8 + 1);
        P.n_prior = np_;
        P.prior_rank0 = rank == 0 ? 1 : 0;
        pb->priors.assign(cons->priors, cons->priors + np_);
    }
    if (cons && cons->n_pair_priors > 0) {
        const int np_ = cons->n_pair_priors;
        std::vector<double> pdat((size_t)np_ * PRIOR_DAT);
        for (int p = 0; p < np_; p++) {
            const aar_pair_prior &q = cons->pair_priors[p];
            memcpy(&pdat[(size_t)p * PRIOR_DAT], q.x6_rel, 6 * sizeof(double));
            memcpy(&pdat[(size_t)p * PRIOR_DAT + 6], q.info, 36 * sizeof(double));
        }
        P.n_pair_el = tp.n_pair_el;
        P.n_pair_items = tp.n_pair_items;
        if ((rc = dev_upload(pb, &P.pair_ends, tp.pair_ends)) || (rc = dev_upload(pb, &P.pair_dat, pdat)) || (rc = dev_upload(pb, &P.pair_el_ent, tp.pair_el_ent)) ||
            (rc = dev_upload(pb, &P.pair_el_start, tp.pair_el_start)) || (rc = dev_upload(pb, &P.pair_el_item, tp.pair_el_item)))
            return rc;
        AL(pair_rec_ws, (size_t)np_ * 54);
        AL(pair_out, (size_t)np_ * 8 + 1);
        P.n_pair = np_;
        P.prior_rank0 = rank == 0 ? 1 : 0;
    }
    return AAR_OK;
}
#undef AL

// ---- step 12: the exchange buffers, the host's result record, and the warm-up copy ----
int finish_uploads(aar_problem *pb) {
    DeviceProblem &P = pb->P;
    const int A = P.A, F = P.F, Fg = pb->L.F;
    int rc;
    if ((rc = dev_alloc(pb, &pb->d_diag, P.n_pad))) return rc;
    if (pb->comm && (rc = dev_alloc(pb, &pb->d_frames_all, 6 * (size_t)std::max(Fg, 1)))) return rc;
    if (pb->comm && (rc = dev_alloc(pb, &pb->d_pack, (size_t)P.n_pad * (P.n_pad + 1) / 2 + 2 * (size_t)P.n_pad + 8))) return rc;
    if (hipHostMalloc((void **)&pb->h_scal, 16 * sizeof(double), hipHostMallocMapped | hipHostMallocCoherent) != hipSuccess)
        return set_error(AAR_ERR_HIP, "hipHostMalloc failed");
    memset(pb->h_scal, 0, 16 * sizeof(double));
    if (hipHostGetDevicePointer((void **)&P.host_result, pb->h_scal, 0) != hipSuccess)
        return set_error(AAR_ERR_HIP, "hipHostGetDevicePointer failed");
    if (hipStreamSynchronize(pb->stream) != hipSuccess) return set_error(AAR_ERR_HIP, "upload failed");
    {   // the runtime brings its device-to-host copy path up on first use (8-13 ms, once per process: scripts/probe/outlier2.py):
        // better here than inside the caller's first solve
        if (pb->h_z.reserve((size_t)6 * (A + F))) return set_error(AAR_ERR_HIP, "hipHostMalloc(pose staging) failed");
        if (hipEventCreateWithFlags(&pb->up_ev, hipEventDisableTiming) != hipSuccess) { pb->up_ev = nullptr; (void)hipGetLastError(); }
        if (hipMemcpyAsync(pb->h_z.data(), P.z[0], (size_t)6 * (A + F) * sizeof(double), hipMemcpyDeviceToHost, pb->stream) != hipSuccess ||
            hipStreamSynchronize(pb->stream) != hipSuccess)
            return set_error(AAR_ERR_HIP, "device-to-host copy failed");
    }
    return AAR_OK;
}

}  // namespace

// cons: validated and not empty, or NULL
static int problem_create(const aar_problem_desc *d, const aar_solver_options *opts, const aar_problem_constraints *cons, aar_problem **out) {
    if (!d || !out) return set_error(AAR_ERR_INVALID, "aar_problem_create: null argument");
    CreateEnv E;
    int rc = read_create_options(opts, E);                                   // 1. options struct and environment
    if (rc) return rc;
    std::vector<int64_t> per_frame;
    int64_t global_slots = 0;
    if ((rc = validate_and_count(d, per_frame, global_slots))) return rc;   // 2. validation and counting
    if ((rc = ensure_device(d->device_id))) return rc;                      // 3. device, streams and events
    aar_problem *pb = new aar_problem();
    auto fail = [&](int code) { aar_problem_destroy(pb); return code; };
    if ((rc = open_streams(d, E, pb))) return fail(rc);
    if ((rc = plan_shard(d, per_frame, pb))) return fail(rc);               // 4. shard range
    DeviceProblem &P = pb->P;
    FramePlan fp = plan_frames(*d, pb->L, per_frame, pb->f_begin, pb->f_end, pb->o_begin);   // 5. frame stage
    P.max_kf = fp.max_kf;
    P.total_slots = fp.total_slots;
    int local_rc = fp.status;   // rank-local limits: decided collectively below
    const std::vector<int32_t> held = plan_held_entities(pb->L, cons);
    const bool held_extra = std::find(held.begin(), held.end(), 1) != held.end();
    bool schur_mfma = false;
    choose_solver(pb, E, global_slots, held_extra, local_rc, schur_mfma);   // 6. solver choice and limits
    if ((rc = agree_on_status(pb, local_rc))) return fail(rc);              // 7. collective agreement
    PlanKnobs knobs = E.knobs;
    knobs.deterministic = P.deterministic != 0; knobs.schur_mfma = schur_mfma; knobs.use_pcg = P.use_pcg != 0; knobs.n_cus = P.n_cus;
    TablePlan tp = plan_tables(pb->L, fp, cons, knobs);                     // 8. table stage
    if ((rc = upload_plan(pb, d, fp, tp))) return fail(rc);                 // 9. upload
    if ((rc = alloc_workspaces(pb, E, tp.sp_total))) return fail(rc);       // 10. workspaces
    if ((rc = upload_priors(pb, cons, tp))) return fail(rc);                // 11. priors
    if ((rc = finish_uploads(pb))) return fail(rc);                         // 12. warm-up copy
    // host copies of the index structure: the plan's own vectors
    pb->h_fslot_start = std::move(fp.fslot_start);
    pb->h_fslot_ent = std::move(fp.fslot_ent);
    pb->h_ent_fixed = std::move(tp.ent_fixed);
    *out = pb;
    return AAR_OK;
}

int64_t aar_problem_full_len(const aar_problem *pb) { return pb->L.full_len(); }
int64_t aar_problem_num_vars(const aar_problem *pb) { return pb->L.z_len(); }
int64_t aar_problem_local_obs(const aar_problem *pb) { return pb->P.N; }

int aar_problem_set_huber_delta(aar_problem *pb, float delta) {
    if (!pb || !(delta > 0.f)) return set_error(AAR_ERR_INVALID, "aar_problem_set_huber_delta: bad argument");
    pb->hubber_delta = delta;
    if (pb->with_huber) pb->P.huber = delta;
    return AAR_OK;
}
float aar_problem_get_huber_delta(const aar_problem *pb) { return pb ? pb->hubber_delta : 0.f; }

int aar_eval_residuals(aar_problem *pb, const double *x_full, double *r, double *sum_sq) {
    if (!pb || !x_full) return set_error(AAR_ERR_INVALID, "aar_eval_residuals: null argument");
    if (r && pb->comm) return set_error(AAR_ERR_UNSUPPORTED, "residual vector output is single-GPU only");
    HIP_TRY(hipSetDevice(pb->device));
    DeviceProblem &P = pb->P;
    int rc = upload_z(pb, x_full, pb->cur);
    if (rc) return rc;
    double *d_r = nullptr;
    if (r) HIP_TRY(hipMalloc((void **)&d_r, std::max<size_t>(1, 8 * (size_t)P.N) * sizeof(double)));
    launch_unpack(P, pb->cur, pb->stream);
    launch_residual(P, pb->cur, d_r, pb->stream);
    HIP_TRY(hipMemsetAsync(P.lin_part, 0, 2 * (size_t)(P.F + 1) * sizeof(double), pb->stream));
    launch_reduce_scalars(P, residual_blocks(P), false, 0ull, pb->stream);
    rc = allreduce(pb, P.scal, 1, NCCL_SUM);
    if (rc) { if (d_r) (void)hipFree(d_r); return rc; }
    pb->seq++;
    launch_publish(P, pb->seq, pb->stream);
    HIP_TRY(hipStreamSynchronize(pb->stream));
    if (r && (rc = copy_d2h(pb, r, d_r, 8 * (size_t)P.N * sizeof(double)))) { (void)hipFree(d_r); return rc; }
    if ((rc = wait_result(pb))) { if (d_r) (void)hipFree(d_r); return rc; }
    if (d_r) (void)hipFree(d_r);
    if (sum_sq) *sum_sq = pb->h_scal[0];
    pb->lm_ready = false;
    return check_async("residual kernels");
}

int aar_reproj_stats(aar_problem *pb, const double *x_full, double *rmse, double *sum_sq) {
    if (!pb) return set_error(AAR_ERR_INVALID, "aar_reproj_stats: null argument");
    const int saved = pb->P.res_f32;
    const float saved_h = pb->P.huber;
    pb->P.res_f32 = 0;
    pb->P.huber = -1.f;
    double ss = 0;
    int rc = aar_eval_residuals(pb, x_full, nullptr, &ss);
    pb->P.res_f32 = saved;
    pb->P.huber = saved_h;
    if (rc) return rc;
    if (sum_sq) *sum_sq = ss;
    if (rmse) *rmse = std::sqrt(ss / (4.0 * (double)pb->N_global));
    return AAR_OK;
}

int aar_eval_normal_equations(aar_problem *pb, const double *x_full, double *JtJ, double *B, double *sum_sq) {
    if (!pb || !x_full) return set_error(AAR_ERR_INVALID, "aar_eval_normal_equations: null argument");
    if (pb->comm) return set_error(AAR_ERR_UNSUPPORTED, "dense normal-equation output is single-GPU only");
    HIP_TRY(hipSetDevice(pb->device));
    DeviceProblem &P = pb->P;
    const PoseLayout &L = pb->L;
    int rc = upload_z(pb, x_full, pb->cur);
    if (rc) return rc;
    if ((rc = zero_block_set(pb, pb->cur))) return rc;
    P.want_w64 = 1;
    rc = eval_blocks(pb, pb->cur, -1.0, -1);
    P.want_w64 = 0;
    if (rc) return rc;
    const int A = P.A, F = P.F, np = P.n_pad;
    const DeviceProblem::Blocks &bk = P.blk[pb->cur];
    std::vector<double> U0((size_t)np * np), g0(np), V((size_t)F * 36), gf((size_t)F * 6), W((size_t)P.total_slots * 36), ep(n_err_terms(P));
    // (copies through the library's page-locked staging, hostcopy.h)
    HIP_TRY(hipStreamSynchronize(pb->stream));
    if ((rc = copy_d2h(pb, U0.data(), bk.S, U0.size() * sizeof(double))) || (rc = copy_d2h(pb, g0.data(), bk.g0, g0.size() * sizeof(double)))) return rc;
    if (F) {
        if ((rc = copy_d2h(pb, V.data(), bk.V, V.size() * sizeof(double))) || (rc = copy_d2h(pb, gf.data(), bk.gf, gf.size() * sizeof(double))) ||
            (rc = copy_d2h(pb, W.data(), bk.W, W.size() * sizeof(double)))) return rc;
    }
    if (!ep.empty() && (rc = copy_d2h(pb, ep.data(), P.err_part, ep.size() * sizeof(double)))) return rc;   // (the frames' sums, then the priors' cost)
    pb->lm_ready = false;
    // reference column of each device parameter (or -1): roots, non-optimised groups and the two idle parameters of an
    // intrinsics entity have none
    const int64_t Pz = L.z_len();
    auto par_col = [&](int a, int i) -> int64_t {
        if (a < L.C) { const int s = L.cam_slot(a); return (s < 0 || !L.oc) ? -1 : L.z_cam0() + 6LL * s + i; }
        if (a < L.C + L.M) { const int s = L.mk_slot(a - L.C); return (s < 0 || !L.om) ? -1 : L.z_mk0() + 6LL * s + i; }
        return i < 4 ? L.z_intr0() + 9LL * (a - L.C - L.M) + i : -1;   // fx cx fy cy; the d0..d4 columns stay zero
    };
    if (JtJ) {
        std::fill(JtJ, JtJ + Pz * Pz, 0.0);
        for (int a = 0; a < A; a++)
            for (int b = 0; b <= a; b++)
                for (int i = 0; i < 6; i++)
                    for (int j = 0; j < 6; j++) {
                        if (a == b && j > i) continue;
                        const int64_t ca = par_col(a, i), cb = par_col(b, j);
                        if (ca < 0 || cb < 0) continue;
                        const double v = U0[(size_t)(6 * a + i) * np + 6 * b + j];
                        JtJ[ca * Pz + cb] = v;
                        JtJ[cb * Pz + ca] = v;
                    }
        if (L.of)
            for (int f = 0; f < F; f++) {
                const int64_t cf = L.z_fr0() + 6LL * f;
                for (int i = 0; i < 6; i++)
                    for (int j = 0; j < 6; j++) JtJ[(cf + i) * Pz + cf + j] = V[(size_t)f * 36 + i * 6 + j];
                for (int s = pb->h_fslot_start[f]; s < pb->h_fslot_start[f + 1]; s++)
                    for (int i = 0; i < 6; i++) {
                        const int64_t ca = par_col(pb->h_fslot_ent[s], i);
                        if (ca < 0) continue;
                        for (int j = 0; j < 6; j++) {
                            const double v = W[(size_t)s * 36 + i * 6 + j];
                            JtJ[ca * Pz + cf + j] = v;
                            JtJ[(cf + j) * Pz + ca] = v;
                        }
                    }
            }
    }
    if (B) {
        std::fill(B, B + Pz, 0.0);
        for (int a = 0; a < A; a++)
            for (int i = 0; i < 6; i++) {
                const int64_t ca = par_col(a, i);
                if (ca >= 0) B[ca] = g0[6 * (size_t)a + i];
            }
        if (L.of)
            for (int f = 0; f < F; f++)
                for (int i = 0; i < 6; i++) B[L.z_fr0() + 6LL * f + i] = gf[(size_t)f * 6 + i];
    }
    if (sum_sq) {
        double s = 0;
        for (double v : ep) s += v;
        *sum_sq = s;
    }
    return AAR_OK;
}

int aar_problem_eval_priors(aar_problem *pb, const double *x_full, double *e_out, double *cost) {
    if (!pb || !x_full) return set_error(AAR_ERR_INVALID, "aar_problem_eval_priors: null argument");
    HIP_TRY(hipSetDevice(pb->device));
    DeviceProblem &P = pb->P;
    if (P.n_prior == 0) {
        if (cost) *cost = 0.0;
        return AAR_OK;
    }
    int rc = upload_z(pb, x_full, pb->cur);
    if (rc) return rc;
    // the entity rows of `cur` are rewritten: whatever the LM state was, it is gone
    pb->lm_ready = false;
    pb->blocks_valid = false;
    launch_unpack(P, pb->cur, pb->stream);
    launch_prior(P, pb->cur, /*add=*/false, pb->stream);
    pb->launches += 2;
    if ((rc = check_async("prior kernels"))) return rc;
    HIP_TRY(hipStreamSynchronize(pb->stream));
    std::vector<double> h((size_t)P.n_prior * 8 + 1);
    if ((rc = copy_d2h(pb, h.data(), P.prior_out, h.size() * sizeof(double)))) return rc;
    if (e_out)
        for (int p = 0; p < P.n_prior; p++) memcpy(e_out + 6 * (size_t)p, &h[8 * (size_t)p], 6 * sizeof(double));
    if (cost) *cost = h[(size_t)P.n_prior * 8];
    return AAR_OK;
}

int aar_problem_eval_pair_priors(aar_problem *pb, const double *x_full, double *e_out, double *cost) {
    if (!pb || !x_full) return set_error(AAR_ERR_INVALID, "aar_problem_eval_pair_priors: null argument");
    HIP_TRY(hipSetDevice(pb->device));
    DeviceProblem &P = pb->P;
    if (P.n_pair == 0) {
        if (cost) *cost = 0.0;
        return AAR_OK;
    }
    int rc = upload_z(pb, x_full, pb->cur);
    if (rc) return rc;
    // the entity rows of `cur` are rewritten: whatever the LM state was, it is gone
    pb->lm_ready = false;
    pb->blocks_valid = false;
    launch_unpack(P, pb->cur, pb->stream);
    launch_pair_prior(P, pb->cur, /*add=*/false, pb->stream);
    pb->launches += 2;
    if ((rc = check_async("pair prior kernels"))) return rc;
    HIP_TRY(hipStreamSynchronize(pb->stream));
    std::vector<double> h((size_t)P.n_pair * 8 + 1);
    if ((rc = copy_d2h(pb, h.data(), P.pair_out, h.size() * sizeof(double)))) return rc;
    if (e_out)
        for (int p = 0; p < P.n_pair; p++) memcpy(e_out + 6 * (size_t)p, &h[8 * (size_t)p], 6 * sizeof(double));
    if (cost) *cost = h[(size_t)P.n_pair * 8];
    return AAR_OK;
}

// T_a^-1 T_b of two poses given as (rvec, t), as (rvec, t): what aar_pair_prior.x6_rel holds.  Host code.
int aar_relative_pose(const double *x6_a, const double *x6_b, double *x6_rel_out) {
    if (!x6_a || !x6_b || !x6_rel_out) return set_error(AAR_ERR_INVALID, "aar_relative_pose: null argument");
    aar::rigid_to_pose(aar::compose(aar::inverse(aar::pose_to_rigid(x6_a)), aar::pose_to_rigid(x6_b)), x6_rel_out);
    return AAR_OK;
}

int aar_eval_damped_step(aar_problem *pb, const double *x_full, double mu, double *delta) {
    if (!pb || !x_full || !delta) return set_error(AAR_ERR_INVALID, "aar_eval_damped_step: null argument");
    HIP_TRY(hipSetDevice(pb->device));
    const PoseLayout &L = pb->L;
    int rc = upload_z(pb, x_full, pb->cur);
    if (rc) return rc;
    if ((rc = zero_block_set(pb, pb->cur))) return rc;
    if ((rc = eval_blocks(pb, pb->cur, -1.0, -1))) return rc;
    pb->vinv_mu = -1;
    pb->schur_mu = -1;
    pb->s_reduced = pb->trial_reduced = false;
    pb->spcg_skip = pb->spcg_backoff = 0;   // (a one-off solve: the problem's own solver gets its chance whatever an earlier LM run ended with)
    pb->last_cg_its = -1;
    pb->near_cap_tries = 0;
    pb->P.spcg_coarse_on = 0;
    pb->P.pcg_e_age = 0;
    if (pb->P.use_pcg && pb->P.pcg_counter) HIP_TRY(hipMemsetAsync(pb->P.pcg_counter + 2, 0, sizeof(int32_t), pb->stream));   // (k_pcgf's coarse space joins by the previous solve's count)
    pb->P.pcg_eta_now = pb->P.pcg_eta;      // (... and the forcing term itself, not the LM's forcing sequence)
    if ((rc = damped_try_fb(pb, mu, false))) return rc == TRY_NOT_POSITIVE_DEFINITE ? AAR_ERR_NUMERIC : rc;
    pb->lm_ready = false;
    std::vector<double> x0(x_full, x_full + L.full_len()), x1(x0);
    if ((rc = download_z(pb, 1 - pb->cur, x1.data()))) return rc;
    // z ordering of the Config
    std::vector<double> z0((size_t)std::max<int64_t>(L.z_len(), 1)), z1(z0);
    extract_z(L, x0.data(), z0.data());
    extract_z(L, x1.data(), z1.data());
    for (int64_t i = 0; i < L.z_len(); i++) delta[i] = z1[i] - z0[i];
    return AAR_OK;
}

// (J^T J)^-1 at x_full: the DIRECT chain's blocks at mu = 0, the reduced system factored by the k_ldl_* chain (one padding tile more than the
// LM path uses, so that every real tile's factor stays in Dfac), S^-1 and the frame marginals by cov_kernels.hip.  DESIGN.md section 13.
namespace {
// What the chain leaves behind for its callers: the row mask (PREDICT_* of kernels.h; aar_problem_covariance only asks whether a row is
// masked), where S^-1, 1 / D, the frame blocks and the entities' diagonal blocks lie in the workspace, the summed sum r^2
struct CovChain {
    std::vector<int32_t> mask;
    double *Sinv = nullptr, *Dinv = nullptr, *frame_blocks = nullptr, *diag_blocks = nullptr;
    int32_t *rowmask = nullptr;
    double sum_sq = 0, dmin = INFINITY, dmax = -INFINITY;
    bool frames = false;
};

// The chain of aar_problem_covariance up to the frame blocks (want_frames) and the entities' diagonal blocks (want_diag_blocks), with its
// pivot check: every caller fails on the same systems with the same message
int cov_chain(aar_problem *pb, const double *x_full, bool want_frames, bool want_diag_blocks, CovChain &out) {
    DeviceProblem &P = pb->P;
    const PoseLayout &L = pb->L;
    const int cur = pb->cur, np = P.n_pad, n2 = P.n_pad + CHOL_NB, nT2 = P.nT + 1, NB = CHOL_NB;
    int rc = upload_z(pb, x_full, cur);
    if (rc) return rc;
    if ((rc = zero_block_set(pb, cur))) return rc;
    // whatever the LM state was, it is gone: the blocks of `cur` are rebuilt and eliminated below
    pb->lm_ready = false;
    pb->blocks_valid = false;
    pb->vinv_mu = pb->schur_mu = -1;
    pb->s_reduced = pb->trial_reduced = false;
    pb->spec_chol_blk = -1;
    if (pb->panels_blk == cur) pb->panels_blk = -1;
    P.want_w64 = 1;   // (the frame kernel reads the fp64 W blocks whatever the problem's solver)
    rc = eval_blocks(pb, cur, -1.0, -1);
    P.want_w64 = 0;
    if (rc) return rc;
    // Schur complement at mu = 0 and this rank's sum r^2 behind g0: they travel in the DIRECT chain's all-reduce
    launch_frame_inv(P, cur, 0.0, pb->stream);
    launch_schur(P, cur, 1.0, pb->stream, 0, 0, nullptr, false);
    launch_reduce_scalars(P, n_err_terms(P), false, 0ull, pb->stream, P.blk[cur].tail);
    pb->launches += 3;
    if (pb->comm && (rc = allreduce_system(pb, cur, 1))) return rc;
    // workspace: staged system with its factor pieces | L | X = L^-1 | S^-1 | 1/D | frame blocks; masks and flags
    const size_t fr = (size_t)std::max(P.F, 1) * 36;
    const size_t o_S2 = 0, o_D = o_S2 + (size_t)n2 * n2 + 2 * (size_t)n2 + 8, o_Li = o_D + (size_t)nT2 * NB * NB, o_Lp = o_Li + (size_t)nT2 * (NB / 16) * 256,
                 o_zf = o_Lp + (size_t)nT2 * n2 * NB, o_ds = o_zf + n2, o_Lc = o_ds + n2, o_X = o_Lc + (size_t)np * np, o_Si = o_X + (size_t)np * np,
                 o_Dv = o_Si + (size_t)np * np, o_fr = o_Dv + np, o_db = o_fr + fr, total = o_db + 36 * (size_t)std::max(P.A, 1);
    if (!pb->cov_ws) {
        if ((rc = dev_alloc(pb, &pb->cov_ws, total))) return rc;
        if ((rc = dev_alloc(pb, &pb->cov_iws, (size_t)np + nT2 + 4))) return rc;
    }
    double *ws = pb->cov_ws;
    int32_t *rowmask = pb->cov_iws, *bsf = rowmask + np, *flg = bsf + nT2;
    // the reduced system's diagonal and the summed sum r^2 on the host: entities no observation touches have an exactly zero diagonal
    HIP_TRY(hipMemcpy2DAsync(pb->d_diag, sizeof(double), P.blk[cur].S, (size_t)(np + 1) * sizeof(double), sizeof(double), np, hipMemcpyDeviceToDevice, pb->stream));
    std::vector<double> diag(np);
    double sum_sq = 0;
    HIP_TRY(hipStreamSynchronize(pb->stream));
    if ((rc = copy_d2h(pb, diag.data(), pb->d_diag, np * sizeof(double))) || (rc = copy_d2h(pb, &sum_sq, P.blk[cur].tail, sizeof(double)))) return rc;
    auto par_col = [&](int a, int i) -> int64_t {   // z column of device parameter (a, i), or -1 (as aar_eval_normal_equations)
        if (a < L.C) { const int s = L.cam_slot(a); return (s < 0 || !L.oc) ? -1 : L.z_cam0() + 6LL * s + i; }
        if (a < L.C + L.M) { const int s = L.mk_slot(a - L.C); return (s < 0 || !L.om) ? -1 : L.z_mk0() + 6LL * s + i; }
        return i < 4 ? L.z_intr0() + 9LL * (a - L.C - L.M) + i : -1;
    };
    std::vector<int32_t> mask(np, 1);
    for (int a = 0; a < P.A; a++) {
        bool seen = false;
        for (int i = 0; i < 6; i++) seen |= par_col(a, i) >= 0 && diag[6 * a + i] != 0.0;
        const bool held = a < L.C + L.M && pb->h_ent_fixed[a];   // (fixed by the caller: as a root)
        // a row without an unknown: a constant (no z column, or held), or -- PREDICT_UNSEEN -- a free parameter nothing determines
        for (int i = 0; i < 6; i++)
            mask[6 * a + i] = (seen && !held && par_col(a, i) >= 0) ? PREDICT_LIVE : ((!held && par_col(a, i) >= 0) ? PREDICT_UNSEEN : PREDICT_CONST);
    }
    if ((rc = copy_h2d(pb, rowmask, mask.data(), np * sizeof(int32_t)))) return rc;
    // factor the staged system with the LM path's own chain: a copy of the problem description pointed at the workspace
    double *S2 = ws + o_S2;
    launch_cov_stage(P.blk[cur].S, np, S2, n2, rowmask, pb->stream);
    HIP_TRY(hipMemsetAsync(S2 + (size_t)n2 * n2, 0, (2 * (size_t)n2 + 8) * sizeof(double), pb->stream));
    HIP_TRY(hipMemsetAsync(bsf, 0, (nT2 + 4) * sizeof(int32_t), pb->stream));
    DeviceProblem Q = P;
    Q.n_pad = n2; Q.nT = nT2;
    Q.blk[cur].S = S2; Q.blk[cur].rhs = S2 + (size_t)n2 * n2; Q.blk[cur].g0 = Q.blk[cur].rhs + n2; Q.blk[cur].tail = Q.blk[cur].g0 + n2;
    Q.Dfac = ws + o_D; Q.Linv16 = ws + o_Li; Q.Lp = ws + o_Lp; Q.zf = ws + o_zf; Q.delta_s = ws + o_ds; Q.bs_flags = bsf; Q.bs_epoch = 0; Q.flags = flg;
    launch_chol(Q, cur, 0.0, pb->stream);
    launch_cov_inverse(S2, Q.Dfac, Q.Lp, np, n2, nT2, P.tune.fused_panel, ws + o_Lc, ws + o_Dv, ws + o_X, ws + o_Si, pb->stream);
    const bool frames = want_frames && L.of && P.F > 0;
    if (frames) launch_cov_frames(P, cur, ws + o_Si, rowmask, ws + o_fr, pb->stream);
    if (want_diag_blocks) launch_cov_diag_blocks(ws + o_Si, np, P.A, ws + o_db, pb->stream);
    pb->launches += 4 + 3 * nT2 + np / 32;
    if ((rc = check_async("covariance kernels"))) return rc;
    HIP_TRY(hipStreamSynchronize(pb->stream));
    HIP_TRY(hipMemsetAsync(P.flags, 0, 4 * sizeof(int32_t), pb->stream));   // (k_frame_inv flags the frames without observations)
    std::vector<double> dinv(np);
    if ((rc = copy_d2h(pb, dinv.data(), ws + o_Dv, np * sizeof(double)))) return rc;
    double dmin = INFINITY, dmax = -INFINITY;
    for (int r = 0; r < np; r++) {
        if (mask[r]) continue;
        const double d = 1.0 / dinv[r];
        if (!(d > 0.0) || !std::isfinite(d)) {
            const int a = r / 6;
            if (a < L.C) return set_error(AAR_ERR_NUMERIC, "covariance: non-positive pivot %g at parameter %d of camera index %d", d, r % 6, a);
            if (a < L.C + L.M) return set_error(AAR_ERR_NUMERIC, "covariance: non-positive pivot %g at parameter %d of marker index %d", d, r % 6, a - L.C);
            return set_error(AAR_ERR_NUMERIC, "covariance: non-positive pivot %g at intrinsic %d of camera index %d", d, r % 6, a - L.C - L.M);
        }
        dmin = std::min(dmin, d);
        dmax = std::max(dmax, d);
    }
    out.mask.swap(mask);
    out.Sinv = ws + o_Si; out.Dinv = ws + o_Dv; out.frame_blocks = ws + o_fr; out.diag_blocks = ws + o_db;
    out.rowmask = rowmask;
    out.sum_sq = sum_sq; out.dmin = dmin; out.dmax = dmax;
    out.frames = frames;
    return AAR_OK;
}
}  // namespace

int aar_problem_covariance(aar_problem *pb, const double *x_full, double *entity_cov, double *entity_diag, double *frame_cov,
                           aar_covariance_report *report) {
    if (!pb || !x_full) return set_error(AAR_ERR_INVALID, "aar_problem_covariance: null argument");
    if (report && report->struct_size < sizeof(uint32_t)) return set_error(AAR_ERR_INVALID, "aar_problem_covariance: report->struct_size not set");
    HIP_TRY(hipSetDevice(pb->device));
    DeviceProblem &P = pb->P;
    const PoseLayout &L = pb->L;
    const int np = P.n_pad;
    CovChain ch;
    int rc = cov_chain(pb, x_full, frame_cov != nullptr, entity_diag && !entity_cov, ch);
    if (rc) return rc;
    const std::vector<int32_t> &mask = ch.mask;
    const bool frames = ch.frames;
    const double sum_sq = ch.sum_sq, dmin = ch.dmin, dmax = ch.dmax;
    auto par_col = [&](int a, int i) -> int64_t {   // z column of device parameter (a, i), or -1 (as aar_eval_normal_equations)
        if (a < L.C) { const int s = L.cam_slot(a); return (s < 0 || !L.oc) ? -1 : L.z_cam0() + 6LL * s + i; }
        if (a < L.C + L.M) { const int s = L.mk_slot(a - L.C); return (s < 0 || !L.om) ? -1 : L.z_mk0() + 6LL * s + i; }
        return i < 4 ? L.z_intr0() + 9LL * (a - L.C - L.M) + i : -1;
    };
    const int64_t Pz = L.z_len(), Fz = L.of ? 6LL * L.F : 0, Pe = Pz - Fz;
    if (entity_cov || entity_diag) {
        // the whole of S^-1 for a dense output; the entities' 6x6 diagonal blocks alone otherwise (an intrinsics entity's 9x9 block is its 4x4
        // inside one 6x6 block: NaN elsewhere)
        std::vector<double> Si((size_t)np * np), db;
        if (entity_cov) {
            if ((rc = copy_d2h(pb, Si.data(), ch.Sinv, Si.size() * sizeof(double)))) return rc;
        } else {
            db.resize(36 * (size_t)std::max(P.A, 1));
            if ((rc = copy_d2h(pb, db.data(), ch.diag_blocks, db.size() * sizeof(double)))) return rc;
        }
        std::vector<int> zdev((size_t)std::max<int64_t>(Pe, 1), -1);   // entity z column -> device row (-1: NaN)
        for (int a = 0; a < P.A; a++)
            for (int i = 0; i < 6; i++) {
                const int64_t zc = par_col(a, i);
                if (zc < 0 || mask[6 * a + i]) continue;
                zdev[(size_t)((L.of && zc >= L.z_fr0()) ? zc - Fz : zc)] = 6 * a + i;
            }
        auto val = [&](int64_t i, int64_t j) -> double {
            const int r = zdev[i], c = zdev[j];
            if (r < 0 || c < 0) return NAN;
            if (!entity_cov) return r / 6 == c / 6 ? db[(size_t)(r / 6) * 36 + (r % 6) * 6 + c % 6] : NAN;   // (only diagonal blocks are asked for)
            return r >= c ? Si[(size_t)r * np + c] : Si[(size_t)c * np + r];
        };
        if (entity_cov)
            for (int64_t i = 0; i < Pe; i++)
                for (int64_t j = 0; j < Pe; j++) entity_cov[i * Pe + j] = val(i, j);
        if (entity_diag) {   // z order: 6 x 6 per camera / marker, 9 x 9 per intrinsics entity
            int64_t z = 0, o = 0;
            while (z < Pe) {
                const int b = (L.oi && z >= Pe - 9LL * L.C) ? 9 : 6;
                for (int i = 0; i < b; i++)
                    for (int j = 0; j < b; j++) entity_diag[o + i * b + j] = val(z + i, z + j);
                z += b;
                o += (int64_t)b * b;
            }
        }
    }
    if (frames && (rc = copy_d2h(pb, frame_cov + 36 * (size_t)pb->f_begin, ch.frame_blocks, (size_t)P.F * 36 * sizeof(double)))) return rc;
    if (report) {
        aar_covariance_report r;
        memset(&r, 0, sizeof r);
        r.struct_size = report->struct_size;
        r.num_residuals = 8 * pb->N_global;
        r.num_vars = Pz;
        r.sum_sq = sum_sq;
        r.sigma2 = r.num_residuals > Pz ? sum_sq / (double)(r.num_residuals - Pz) : NAN;
        r.min_pivot = dmin;
        r.max_pivot = dmax;
        r.frames_written = frames ? P.F : 0;
        memcpy(report, &r, std::min<size_t>(report->struct_size, sizeof r));
    }
    return check_async("covariance");
}

// Residual report: e_d and the first digit's histogram in one pass over ordering A, an exact radix select of the
// lower median on the device (RR_PASSES histogram / pick pairs, no host round trip on one GPU; with a communicator every histogram is
// all-reduced as doubles, so every rank picks the same digits), then keep flags and the run / entity sums in a fixed order.
namespace {
int rr_setup(aar_problem *pb) {
    DeviceProblem &P = pb->P;
    RRWork &w = pb->rr;
    const int64_t N = P.N;
    const int C = P.C, M = P.M;
    // ordering B as the problem built it: rebuilt by the planner's own function (host/problem_plan.h) from the device's ordering A,
    // its (camera, marker) runs and their lists per camera / marker
    std::vector<ObsIdx> a_idx((size_t)N);
    int rc;
    if (N && (rc = copy_d2h(pb, a_idx.data(), P.a_idx, (size_t)N * sizeof(ObsIdx)))) return rc;
    const OrderingB B = plan_ordering_b(a_idx.data(), N);
    const std::vector<int32_t> &perm = B.perm, &run_start = B.run_start;
    const int R = (int)run_start.size() - 1;
    std::vector<int32_t> run_mk(R), cam_run_start(C + 1, 0), mk_run_start(M + 1, 0), mk_runs;
    for (int r = 0; r < R; r++) {
        const ObsIdx &h = a_idx[perm[run_start[r]]];
        cam_run_start[h.cam + 1]++;
        mk_run_start[h.marker - C + 1]++;
        run_mk[r] = h.marker - C;
    }
    for (int c = 0; c < C; c++) cam_run_start[c + 1] += cam_run_start[c];
    for (int m = 0; m < M; m++) mk_run_start[m + 1] += mk_run_start[m];
    mk_runs.resize(R);
    {
        std::vector<int32_t> fill(mk_run_start.begin(), mk_run_start.end() - 1);
        for (int r = 0; r < R; r++) mk_runs[fill[run_mk[r]]++] = r;   // runs are camera-ascending: so is every marker's list
    }
    w.R = R;
    if ((rc = dev_upload(pb, &w.perm, perm)) || (rc = dev_upload(pb, &w.run_start, run_start)) || (rc = dev_upload(pb, &w.cam_run_start, cam_run_start)) ||
        (rc = dev_upload(pb, &w.mk_run_start, mk_run_start)) || (rc = dev_upload(pb, &w.mk_runs, mk_runs)))
        return rc;
    if ((rc = dev_alloc(pb, &w.err, (size_t)N)) || (rc = dev_alloc(pb, &w.ss, (size_t)N)) || (rc = dev_alloc(pb, &w.keep, (size_t)N)) ||
        (rc = dev_alloc(pb, &w.fstat, 4 * (size_t)P.F)) || (rc = dev_alloc(pb, &w.rstat, 5 * (size_t)R)) || (rc = dev_alloc(pb, &w.rmax, (size_t)R)) ||
        (rc = dev_alloc(pb, &w.esum, 5 * (size_t)(C + M) + 1)) || (rc = dev_alloc(pb, &w.emax, (size_t)(C + M))) ||
        (rc = dev_alloc(pb, &w.hist, (size_t)RR_HIST_WORDS)) || (rc = dev_alloc(pb, &w.hd, (size_t)RR_BINS + 2)) || (rc = dev_alloc(pb, &w.sel, 1)))
        return rc;
    pb->rr_ready = true;
    return AAR_OK;
}

double rr_threshold_host(const aar_outlier_rule *rule, double median) {   // (k_rr_keep's rule, for a problem without detections)
    if (!rule || (rule->k_median <= 0.0 && rule->min_px <= 0.0)) return INFINITY;
    if (rule->k_median <= 0.0) return rule->min_px;
    const double a = rule->k_median * median;
    return a > rule->min_px ? a : rule->min_px;
}
}  // namespace

int aar_problem_residual_report(aar_problem *pb, const double *x_full, const aar_outlier_rule *rule, double *det_err, uint8_t *keep,
                                double *cam_stats, double *marker_stats, double *frame_stats, aar_residual_report *report) {
    if (!pb || !x_full || !report) return set_error(AAR_ERR_INVALID, "aar_problem_residual_report: null argument");
    if (report->struct_size != sizeof(aar_residual_report))
        return set_error(AAR_ERR_INVALID, "aar_problem_residual_report: report->struct_size %u, expected %zu", report->struct_size, sizeof(aar_residual_report));
    if (rule && rule->struct_size != sizeof(aar_outlier_rule))
        return set_error(AAR_ERR_INVALID, "aar_problem_residual_report: rule->struct_size %u, expected %zu", rule->struct_size, sizeof(aar_outlier_rule));
    if (rule && (std::isnan(rule->k_median) || std::isnan(rule->min_px))) return set_error(AAR_ERR_INVALID, "aar_problem_residual_report: NaN in the rule");
    HIP_TRY(hipSetDevice(pb->device));
    DeviceProblem &P = pb->P;
    const int C = P.C, M = P.M, cur = pb->cur;
    aar_residual_report r;
    memset(&r, 0, sizeof r);
    r.struct_size = report->struct_size;
    if (pb->N_global == 0) {   // nothing to select (the same on every rank)
        if (cam_stats) std::fill(cam_stats, cam_stats + 4 * (size_t)C, 0.0);
        if (marker_stats) std::fill(marker_stats, marker_stats + 4 * (size_t)M, 0.0);
        if (frame_stats) std::fill(frame_stats + 4 * (size_t)pb->f_begin, frame_stats + 4 * (size_t)pb->f_end, 0.0);
        r.rmse = r.median = r.max = NAN;
        r.threshold = rr_threshold_host(rule, NAN);
        *report = r;
        return AAR_OK;
    }
    int rc;
    if (!pb->rr_ready && (rc = rr_setup(pb))) return rc;
    const RRWork &w = pb->rr;
    if ((rc = upload_z(pb, x_full, cur))) return rc;
    // whatever the LM state was, it is gone: z[cur] and its entity rows now hold x_full
    pb->lm_ready = false;
    pb->blocks_valid = false;
    pb->vinv_mu = pb->schur_mu = -1;
    pb->s_reduced = pb->trial_reduced = false;
    pb->spec_chol_blk = -1;
    if (pb->panels_blk == cur) pb->panels_blk = -1;
    HIP_TRY(hipMemsetAsync(w.hist, 0, RR_HIST_WORDS * sizeof(uint32_t), pb->stream));
    launch_unpack(P, cur, pb->stream);
    launch_rr_errors(P, cur, w, (unsigned long long)((pb->N_global - 1) / 2), pb->stream);
    for (int pass = 0; pass < RR_PASSES; pass++) {
        if (pass > 0) launch_rr_select_pass(P, w, pb->stream);
        if (pb->comm) {
            launch_rr_to_double(w, pb->stream);
            if ((rc = allreduce(pb, w.hd, RR_BINS + 2, NCCL_SUM))) return rc;
        }
        launch_rr_pick(w, pb->comm != nullptr, pb->stream);
    }
    launch_rr_stats(P, w, rule ? 1 : 0, rule ? rule->k_median : 0.0, rule ? rule->min_px : 0.0, pb->stream);
    pb->launches += 2 + 2 * RR_PASSES + 2 + (w.R > 0 ? 1 : 0) + (pb->comm ? RR_PASSES : 0);
    if ((rc = check_async("residual report kernels"))) return rc;
    if (pb->comm && ((rc = allreduce(pb, w.esum, 5 * (size_t)(C + M) + 1, NCCL_SUM)) || (rc = allreduce(pb, w.emax, (size_t)(C + M), NCCL_MAX)))) return rc;
    HIP_TRY(hipStreamSynchronize(pb->stream));
    RRSel sel;
    std::vector<double> esum(5 * (size_t)(C + M) + 1), emax((size_t)(C + M));
    if ((rc = copy_d2h(pb, &sel, w.sel, sizeof sel)) || (rc = copy_d2h(pb, esum.data(), w.esum, esum.size() * sizeof(double))) ||
        (rc = copy_d2h(pb, emax.data(), w.emax, emax.size() * sizeof(double))))
        return rc;
    if (!sel.done) return set_error(AAR_ERR_HIP, "residual report: the select did not converge (rank %llu left at bit %d)", sel.rank, sel.pshift);
    if (det_err && P.N && (rc = copy_d2h(pb, det_err, w.err, (size_t)P.N * sizeof(double)))) return rc;
    if (keep && P.N && (rc = copy_d2h(pb, keep, w.keep, (size_t)P.N))) return rc;
    if (frame_stats && P.F && (rc = copy_d2h(pb, frame_stats + 4 * (size_t)pb->f_begin, w.fstat, 4 * (size_t)P.F * sizeof(double)))) return rc;
    double mx = 0.0;
    int64_t n_nan = 0;
    for (int e = 0; e < C + M; e++) {
        const double *q = &esum[5 * (size_t)e];
        const double emx = q[4] > 0 ? NAN : emax[e];
        double *out = e < C ? (cam_stats ? cam_stats + 4 * (size_t)e : nullptr) : (marker_stats ? marker_stats + 4 * (size_t)(e - C) : nullptr);
        if (out) { out[0] = q[0]; out[1] = q[1]; out[2] = emx; out[3] = q[2]; }
        const bool emptied = q[0] > 0 && q[2] == q[0];
        if (e < C) {   // every detection belongs to exactly one camera: the totals are the cameras' sums, ascending
            r.num_detections += (int64_t)q[0];
            r.num_rejected += (int64_t)q[2];
            r.num_nonfinite += (int64_t)q[3];
            n_nan += (int64_t)q[4];
            r.sum_sq += q[1];
            mx = std::max(mx, emax[e]);
            r.cams_emptied += emptied;
        } else {
            r.markers_emptied += emptied;
        }
    }
    r.frames_emptied = (int32_t)esum[5 * (size_t)(C + M)];
    r.rmse = std::sqrt(r.sum_sq / (4.0 * (double)r.num_detections));
    uint64_t mk = sel.prefix;
    memcpy(&r.median, &mk, sizeof mk);
    r.max = n_nan > 0 ? NAN : mx;
    r.threshold = sel.t;
    *report = r;
    return AAR_OK;
}

// SparseLevMarq::init, libs/sparselevmarq.h:238-249.  The residual of the start point comes out of the same pass that
// builds its normal equations (the first step() needs them anyway).
int aar_lm_init(aar_problem *pb, const double *x_full, const aar_lm_params *prm) {
    if (!pb || !x_full) return set_error(AAR_ERR_INVALID, "aar_lm_init: null argument");
    HIP_TRY(hipSetDevice(pb->device));
    if (prm) pb->prm = *prm;
    DeviceProblem &P = pb->P;
    pb->cur = 0;
    pb->trial_points = 0;
    pb->launches = 0;
    pb->spcg_skip = pb->spcg_backoff = 0;
    pb->last_cg_its = -1;
    pb->near_cap_tries = 0;
    P.spcg_coarse_on = 0;
    P.pcg_e_age = 0;
    if (P.use_pcg && P.pcg_counter) HIP_TRY(hipMemsetAsync(P.pcg_counter + 2, 0, sizeof(int32_t), pb->stream));   // (k_pcgf's coarse space joins by the previous solve's count)
    if (pb->spec_chol_blk >= 0) {   // a factorisation queued ahead of the last step of the previous solve: its pivot flags mean nothing
        HIP_TRY(hipMemsetAsync(P.flags, 0, 4 * sizeof(int32_t), pb->stream));
        pb->spec_chol_blk = -1;
    }
    memset(&pb->times, 0, sizeof pb->times);
    int rc = upload_z(pb, x_full, 0);
    if (rc) return rc;
    // A solve's fixed cost (every 15 steps or so in a bundle adjustment that converges): the first launch turns z into entity rows AND
    // clears block set 0 and the linear-model partials, pass A clears block set 1 on its way, and max diag(J^T J) of the start point
    // (mu_0, libs/sparselevmarq.h:369-377) comes out of the launch that reduces its sum r^2 -- three launches less than one kernel per job
    if (P.F > 0 && P.n_chunks > 0 && !pb->comm) {
        launch_unpack(P, 0, pb->stream, /*zero_blk=*/0);
        pb->launches += 1;
        if ((rc = eval_blocks(pb, 0, -1.0, /*zero_blk=*/1, /*ents_ready=*/true))) return rc;
    } else {
        if ((rc = zero_for_init(pb))) return rc;
        if ((rc = eval_blocks(pb, 0, -1.0, -1))) return rc;
    }
    pb->huber_of_blocks = P.huber;
    pb->mu_seed_valid = false;
    // (single GPU: mu_0 rides to the host with the sum r^2: the first step() then needs no round trip of its own)
    if ((rc = launch_scalars(pb, n_err_terms(P), pb->comm ? -1 : 0))) return rc;
    // Head start of the first step (single GPU, direct solver): its damping mu_0 = tau * max diag(J^T J) is on the device one kernel before the host
    // can read it, and the frame inverses and the Schur complement need nothing else -- they are queued HERE, with mu_0 read on the device, and
    // run while the record travels to the host and the host queues the factorisation.  (tau changed between init and step: the damped try finds
    // another damping than schur_mu and takes the complement back, as after a mispredicted step.)  AAR_INIT_HEADSTART=0: off.
    const bool headstart = P.tune.init_headstart && !pb->comm && !P.use_pcg && !pb->stage_timers && !pb->profiling && P.F > 0;
    if (headstart) {
        launch_frame_inv(P, 0, 0.0, pb->stream, P.scal + 4, pb->prm.tau);
        launch_schur(P, 0, 1.0, pb->stream, 0, 0, nullptr, false);
        pb->launches += 2;
    }
    if ((rc = wait_result(pb))) return rc;
    if (!pb->comm) { pb->mu_seed = pb->h_scal[4]; pb->mu_seed_valid = true; }
    pb->currErr = pb->prevErr = pb->h_scal[0];
    pb->rel_drop = -1;
    pb->blocks_valid = true;
    pb->vinv_mu = -1;
    pb->schur_mu = -1;
    if (headstart) {
        const double mu0 = pb->mu_seed * pb->prm.tau;   // (the expression aar_lm_step uses: the same double as the device's tau * scal[4])
        pb->vinv_mu = mu0;
        pb->schur_mu = mu0;
        panels_now(pb, 0, mu0);
    }
    pb->s_reduced = pb->trial_reduced = false;
    pb->mu = -1;
    pb->v = 2;  // indeterminate in the reference (libs/sparselevmarq.h:133); every accepted step sets 2 (:411)
    pb->lm_ready = true;
    return AAR_OK;
}

// SparseLevMarq::step(f, J), libs/sparselevmarq.h:349-430
int aar_lm_step(aar_problem *pb, aar_lm_iter *out) {
    if (!pb) return set_error(AAR_ERR_INVALID, "aar_lm_step: null argument");
    if (!pb->lm_ready) return set_error(AAR_ERR_INVALID, "aar_lm_step: call aar_lm_init first");
    HIP_TRY(hipSetDevice(pb->device));
    int rc;
    // verbose: the reference's per-step stage line (:425) needs per-stage device times, i.e. the stage timers for this step
    struct VerboseTimers {
        aar_problem *pb; bool was; aar_stage_times t0;
        explicit VerboseTimers(aar_problem *p) : pb(p), was(p->stage_timers), t0(p->times) { if (pb->prm.verbose) pb->stage_timers = true; }
        ~VerboseTimers() { pb->stage_timers = was; }
    } vt(pb);
    if (!pb->blocks_valid && (rc = rebuild_current(pb))) return rc;  // J, Jt*J, B at curr_z (:353-367)
    if (pb->mu < 0) {                                                  // first time only (:369-377)
        if (pb->mu_seed_valid && pb->cur == 0 && pb->blocks_valid) pb->mu = pb->mu_seed * pb->prm.tau;   // (the blocks of the start point are still the ones it was taken from)
        else if ((rc = initial_mu(pb, pb->prm.tau, &pb->mu))) return rc;
        pb->mu_seed_valid = false;
    }
    double gain = 0, dnorm = 0;
    int ntries = 0;
    bool accepted = false;
    do {
        if (!pb->blocks_valid && (rc = rebuild_current(pb))) return rc;  // a rejected try consumed them
        const double mu_used = pb->mu;
        if (pb->P.use_pcg || pb->P.use_spcg)   // (every rank sees the same errors: the same choice)
            pb->P.pcg_eta_now = (pb->P.pcg_eta_loose > pb->P.pcg_eta && (pb->rel_drop < 0 || pb->rel_drop > pb->P.pcg_eta_switch)) ? pb->P.pcg_eta_loose : pb->P.pcg_eta;
        if ((rc = damped_try_fb(pb, mu_used, true))) {
            if (rc != TRY_NOT_POSITIVE_DEFINITE) return rc;
            // J^T J + mu I came out indefinite in floating point: the reference's LDL^T would hand back the stationary point
            // of an indefinite model and its gain test would reject the trial (libs/sparselevmarq.h:408-419); same outcome here
            pb->mu = mu_used * pb->v;
            pb->v = pb->v * 5;
            pb->trial_reduced = false;
            pb->blocks_valid = false;
            gain = -1;
            continue;
        }
        const double *sc = pb->h_scal;
        const double err = sc[0];
        // L = 0.5 * delta^T (mu*delta - B) (:406); frame pieces were summed over ranks; the shared-parameter pieces
        // |delta_s|^2 and delta_s . g0 are computed from replicated data (g0 was all-reduced with S) and counted once
        const double d2 = sc[1] + sc[5];
        const double dg = (pb->P.use_pcg && pb->comm) ? sc[2] : sc[2] + sc[6];   // (PCG with ranks: the shared piece is inside the rank sum)
        const double Lq = 0.5 * (mu_used * d2 - dg);
        dnorm = std::sqrt(d2);
        gain = (err - pb->prevErr) / Lq;
        if (gain > 0 && ((err - pb->prevErr) < 0)) {  // :409-415
            pb->mu = mu_used * std::max(0.33, 1. - std::pow(2 * gain - 1, 3));
            pb->v = 2.f;
            pb->rel_drop = pb->prevErr > 0 ? (pb->prevErr - err) / pb->prevErr : 0.0;
            pb->currErr = err;
            pb->cur = 1 - pb->cur;  // curr_z = estimated_z; its blocks were built speculatively by the try
            pb->huber_of_blocks = pb->P.huber;
            pb->vinv_mu = mu_used * 0.33;   // what pass A inverted for
            pb->schur_mu = mu_used * 0.33;  // ... and what the speculative Schur complement was taken with
            pb->s_reduced = pb->trial_reduced;   // multi-GPU: ... and whether it has been all-reduced already
            pb->trial_reduced = false;
            pb->blocks_valid = true;        // (a damping other than the predicted one is repaired in damped_try)
            accepted = true;
        } else {
            pb->mu = mu_used * pb->v;
            pb->v = pb->v * 5;
            pb->trial_reduced = false;
        }
    } while (gain <= 0 && ntries++ < 5 && !accepted);
    if (out) {
        out->err = pb->currErr; out->mu = pb->mu; out->gain = gain; out->delta_norm = dnorm;
        out->accepted = accepted ? 1 : 0;
        out->tries = ntries + (accepted ? 1 : 0);
    }
    if (pb->prm.verbose) {
        fprintf(stderr, "Curr Error=%.5g AErr(prev-curr)=%.5g gain=%.5g dumping factor=%.5g\n", pb->currErr,
                (pb->prevErr - pb->currErr) / (8.0 * (double)pb->N_global), gain, pb->mu);
        // the reference's stage names (libs/sparselevmarq.h:425), seconds.  "J" = the fused residual + Jacobian + block accumulation
        // passes (which ARE transpose, Jt*J and B here: nothing is transposed or multiplied afterwards), "Jt*J" = the reduction of
        // those blocks onto the shared parameters (Schur complement), "chol" = dense LDL^T + both back-substitutions
        const aar_stage_times &a = vt.t0, &b = pb->times;
        fprintf(stderr, " J=%.6g transpose=%.6g Jt*J=%.6g B=%.6g chol=%.6g\n", b.jacobian_normal_eq - a.jacobian_normal_eq, 0.0, b.schur - a.schur, 0.0,
                (b.chol - a.chol) + (b.backsub - a.backsub));
    }
    return AAR_OK;
}

int aar_lm_get_solution(aar_problem *pb, double *x_full, double *err) {
    if (!pb || !x_full) return set_error(AAR_ERR_INVALID, "aar_lm_get_solution: null argument");
    if (!pb->lm_ready) return set_error(AAR_ERR_INVALID, "aar_lm_get_solution: no LM state");
    HIP_TRY(hipSetDevice(pb->device));
    if (err) *err = pb->currErr;
    return download_z(pb, pb->cur, x_full);
}

// SparseLevMarq::solve(z, f, J), libs/sparselevmarq.h:440-472
int aar_lm_solve(aar_problem *pb, double *x_full, const aar_lm_params *prm, aar_lm_report *rep) {
    if (!pb || !x_full) return set_error(AAR_ERR_INVALID, "aar_lm_solve: null argument");
    // MultiCamMapper::solve sets hubberDelta = 10 before solver.solve (libs/multicam_mapper.cpp:425) and installs optCallBack as
    // the step callback (:422).  A with_huber problem WITHOUT a caller's step callback gets exactly that pair here; a caller
    // that installs its own callback (aar::MultiCamMapper does) owns both the start value and the schedule.
    const bool own_schedule = pb->with_huber && !pb->step_cb;
    if (own_schedule) {
        pb->hubber_delta = 10;
        pb->P.huber = pb->hubber_delta;
    }
    int rc = aar_lm_init(pb, x_full, prm);
    if (rc) return rc;
    const auto t0 = std::chrono::steady_clock::now();
    const double rows = 8.0 * (double)pb->N_global;
    const double initial = pb->currErr;
    int mustExit = 0, iters = 0;
    auto after_step = [&](const aar_lm_iter &it) -> int {   // _step_callback(curr_z), :449 / :463
        if (rep && rep->trace && iters < rep->trace_cap) rep->trace[iters] = it;
        iters++;
        if (pb->step_cb) {
            if (pb->step_want_z && (rc = current_z_for_callbacks(pb, x_full))) return rc;
            pb->step_cb(pb->step_ctx, pb->step_want_z ? pb->cb_z.data() : nullptr, pb->L.z_len());
        } else if (own_schedule && pb->hubber_delta > 2.5) {  // optCallBack, libs/multicam_mapper.cpp:412-417 (float -= double)
            pb->hubber_delta = (float)((double)pb->hubber_delta - 7.5 / 500);
            pb->P.huber = pb->hubber_delta;
        }
        return AAR_OK;
    };
    if (pb->stop_fn) {   // :444-450: do { step; callback } while (!stop(curr_z)) -- no iteration cap, no error-based exit
        bool stop = false;
        do {
            aar_lm_iter it;
            if ((rc = aar_lm_step(pb, &it))) return rc;
            if ((rc = after_step(it))) return rc;
            // (prevErr is NOT advanced on this branch of the reference: every gain test keeps comparing with the error of the
            //  start point, libs/sparselevmarq.h:444-450 against :464)
            if ((rc = current_z_for_callbacks(pb, x_full))) return rc;
            stop = pb->stop_fn(pb->stop_ctx, pb->cb_z.data(), pb->L.z_len()) != 0;
        } while (!stop);
    } else {
        for (int i = 0; i < pb->prm.max_iters && !mustExit; i++) {
            aar_lm_iter it;
            if ((rc = aar_lm_step(pb, &it))) return rc;
            if (pb->currErr < pb->prm.min_error) mustExit = 1;
            if (std::fabs(pb->prevErr - pb->currErr) <= pb->prm.min_step_error_diff ||
                std::fabs((pb->prevErr - pb->currErr) / rows) <= pb->prm.min_average_step_error_diff || !it.accepted)
                mustExit = 2;
            if (pb->currErr > pb->prevErr) mustExit = 3;
            if ((rc = after_step(it))) return rc;
            pb->prevErr = pb->currErr;
        }
    }
    // (the last step's speculative work may still be running: only waited for when somebody reads timers)
    const bool lazy = !pb->comm && !pb->profiling && !pb->stage_timers && iters > 0;
    if (!lazy) HIP_TRY(hipStreamSynchronize(pb->stream));
    const double secs = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    pb->times.total = secs;
    pb->times.launches = pb->launches;
    if ((rc = download_z(pb, pb->cur, x_full, lazy))) return rc;
    if (rep) {
        rep->iterations = iters;
        rep->stop_code = mustExit;
        rep->initial_err = initial;
        rep->final_err = pb->currErr;
        rep->final_mu = pb->mu;
        rep->solve_seconds = secs;
        rep->trial_points = pb->trial_points;
    }
    return AAR_OK;
}

int aar_lm_set_step_callback(aar_problem *pb, aar_lm_step_callback fn, void *ctx, int32_t want_z) {
    if (!pb) return set_error(AAR_ERR_INVALID, "aar_lm_set_step_callback: null argument");
    pb->step_cb = fn;
    pb->step_ctx = ctx;
    pb->step_want_z = fn && want_z;
    return AAR_OK;
}

int aar_lm_set_stop_function(aar_problem *pb, aar_lm_stop_function fn, void *ctx) {
    if (!pb) return set_error(AAR_ERR_INVALID, "aar_lm_set_stop_function: null argument");
    pb->stop_fn = fn;
    pb->stop_ctx = ctx;
    return AAR_OK;
}

int aar_problem_extract_z(const aar_problem *pb, const double *x_full, double *z) {
    if (!pb || !x_full || !z) return set_error(AAR_ERR_INVALID, "aar_problem_extract_z: null argument");
    extract_z(pb->L, x_full, z);
    return AAR_OK;
}

int aar_problem_merge_z(const aar_problem *pb, const double *z, double *x_full) {
    if (!pb || !x_full || !z) return set_error(AAR_ERR_INVALID, "aar_problem_merge_z: null argument");
    merge_z(pb->L, z, x_full);
    return AAR_OK;
}

int aar_track(aar_problem *pb, double *x_full, const aar_lm_params *prm, int32_t *iterations, double *final_err) {
    if (!pb || !x_full) return set_error(AAR_ERR_INVALID, "aar_track: null argument");
    HIP_TRY(hipSetDevice(pb->device));
    DeviceProblem &P = pb->P;
    aar_lm_params p;
    if (prm) p = *prm; else aar_lm_default_params(&p);
    pb->lm_ready = false;
    const int F = P.F;
    int rc = upload_z(pb, x_full, pb->cur);
    if (rc) return rc;
    int32_t *d_it = nullptr;
    double *d_err = nullptr;
    HIP_TRY(hipMalloc((void **)&d_it, std::max(F, 1) * sizeof(int32_t)));
    if (hipMalloc((void **)&d_err, std::max(F, 1) * sizeof(double)) != hipSuccess) { (void)hipFree(d_it); return set_error(AAR_ERR_HIP, "hipMalloc failed"); }
    launch_unpack(P, pb->cur, pb->stream);  // rows of the fixed cameras / markers
    launch_track(P, pb->cur, p.max_iters, p.min_error, p.min_step_error_diff, p.min_average_step_error_diff, p.tau, d_it, d_err, pb->stream);
    std::vector<int32_t> h_it(std::max(F, 1));
    std::vector<double> h_err(std::max(F, 1));
    rc = copy_d2h(pb, h_it.data(), d_it, std::max(F, 1) * sizeof(int32_t));
    if (!rc) rc = copy_d2h(pb, h_err.data(), d_err, std::max(F, 1) * sizeof(double));
    (void)hipFree(d_it);
    (void)hipFree(d_err);
    if (rc) return rc;
    if ((rc = check_async("track kernel"))) return rc;
    // only the frame poses move; download_z honours the Config flags, so force "frames on, shared off" for this call
    PoseLayout keep = pb->L;
    pb->L.oc = false; pb->L.om = false; pb->L.of = true;
    rc = download_z(pb, pb->cur, x_full);
    pb->L = keep;
    if (rc) return rc;
    // per-frame outputs are indexed by global frame; a sharded problem returns its own range and zeros elsewhere
    if (iterations) { std::fill(iterations, iterations + pb->L.F, 0); for (int f = 0; f < F; f++) iterations[pb->f_begin + f] = h_it[f]; }
    if (final_err) { std::fill(final_err, final_err + pb->L.F, 0.0); for (int f = 0; f < F; f++) final_err[pb->f_begin + f] = h_err[f]; }
    return AAR_OK;
}

// ------------------------------------------------------------------------------------------------
// Smoothed tracking (smooth_kernels.hip)
// ------------------------------------------------------------------------------------------------
namespace {

// the caller's struct read up to its struct_size; false: too short to hold the sigmas
bool smooth_params_read(const aar_smooth_params *sp, aar_smooth_params *out) {
    memset(out, 0, sizeof *out);
    if (sp->struct_size < offsetof(aar_smooth_params, sigma_trans) + sizeof(double)) return false;
    memcpy(out, sp, std::min<size_t>(sp->struct_size, sizeof *out));
    // the fields appended for the motion model count only when the struct holds them whole
    if (sp->struct_size < offsetof(aar_smooth_params, model) + sizeof(int32_t)) out->model = AAR_SMOOTH_MODEL_RANDOM_WALK;
    if (sp->struct_size < offsetof(aar_smooth_params, sigma_rot0) + sizeof(double)) out->sigma_rot0 = 0.0;
    if (sp->struct_size < offsetof(aar_smooth_params, sigma_trans0) + sizeof(double)) out->sigma_trans0 = 0.0;
    return true;
}

// device memory that one call owns: n_dbl doubles and n_int int32 behind them, zeroed on the problem's stream
struct DevMem {
    double *p = nullptr;
    ~DevMem() { if (p) (void)hipFree(p); }
    int alloc(aar_problem *pb, size_t n_dbl, size_t n_int = 0) {
        const size_t bytes = n_dbl * sizeof(double) + n_int * sizeof(int32_t);
        HIP_TRY(hipMalloc((void **)&p, bytes));
        HIP_TRY(hipMemsetAsync(p, 0, bytes, pb->stream));
        return AAR_OK;
    }
};

// the diagonal, lag-one and lag-two blocks of H^-1 ([F][36] each, on the device; l2 under constant velocity only) and what launching them took
struct SmoothSel {
    double *fc = nullptr, *lc = nullptr, *l2 = nullptr;
    int launches = 0;
};

// One smoother call on the host: the caller's parameters, the motion model and that model's work area.  Every entry
// drives either model through it; the kernels of the two models stay apart behind the two-way branches below.
struct SmoothRun {
    aar_problem *pb = nullptr;
    aar_smooth_params sp;
    bool cv = false;     // AAR_SMOOTH_MODEL_CONSTANT_VELOCITY
    SmoothWork rw;       // carved by begin() out of mem: this one under the random walk ...
    SmoothCvWork cw;     // ... this one under constant velocity
    DevMem mem;

    double *z(int cur) const { return cv ? cw.z[cur] : rw.z[cur]; }
    const double *Ef(int cur) const { return cv ? cw.Ef[cur] : rw.Ef[cur]; }
    const double *Pe(int cur) const { return cv ? cw.Pe[cur] : rw.Pe[cur]; }
    const double *res() const { return cv ? cw.res : rw.res; }
    const int32_t *flag() const { return cv ? cw.flag : rw.flag; }
    const char *elimination() const { return cv ? "block-pentadiagonal" : "block-tridiagonal"; }

    // H, b and costs at z[cur] (with_j), or the trial point z[1 - cur] = z[cur] + delta with its costs: two launches
    void eval(int cur, bool with_j) const {
        if (cv) launch_smooth_cv_eval(pb->P, pb->cur, cw, cur, with_j, pb->stream);
        else launch_smooth_eval(pb->P, pb->cur, rw, cur, with_j, pb->stream);
    }
    // the damped solve; returns its launches
    int solve(double mu) const { return cv ? launch_smooth_cv_solve(cw, pb->P.F, mu, pb->stream) : launch_smooth_solve(rw, pb->P.F, mu, pb->stream); }

    // lambda from the sigmas and the frame times, onto the device (F > 1).  Random walk: [F-1][2], one entry per pair.  Constant velocity:
    // [F][2], entry 0 pair 0 (sigma_rot0 / sigma_trans0), entry f term f, entry F-1 zero
    int upload_lambda(const aar_smooth_params &s) const {
        const int F = pb->P.F;
        std::vector<double> lam(2 * (size_t)(cv ? F : F - 1), 0.0);
        for (int f = 0; f + 1 < F; f++) {
            const double dt = s.frame_time ? s.frame_time[f + 1] - s.frame_time[f] : 1.0;
            const double sr = cv && f == 0 ? s.sigma_rot0 : s.sigma_rot, st = cv && f == 0 ? s.sigma_trans0 : s.sigma_trans;
            lam[2 * (size_t)f] = 1.0 / (sr * sr * dt);
            lam[2 * (size_t)f + 1] = 1.0 / (st * st * dt);
        }
        return copy_h2d(pb, cv ? cw.lam : rw.lam, lam.data(), lam.size() * sizeof(double));
    }

    // What every entry starts its device work with: x_full into the problem's pose vector and, with work, the rows of the fixed cameras and
    // markers, the zeroed work area, lambda with the ratios r_f or the expected motions, and the frame poses in z[0].  Without work (the
    // random-walk query that returns no covariance) the poses stay in the problem's vector and rw stays empty.
    int begin(const double *x_full, bool work = true) {
        HIP_TRY(hipSetDevice(pb->device));
        DeviceProblem &P = pb->P;
        const int F = P.F;
        pb->lm_ready = false;
        pb->blocks_valid = false;
        int rc = upload_z(pb, x_full, pb->cur);
        if (rc || !work) return rc;
        launch_unpack(P, pb->cur, pb->stream);
        if ((rc = mem.alloc(pb, cv ? smooth_cv_work_doubles(F) : smooth_work_doubles(F)))) return rc;
        if (cv) smooth_cv_work_carve(cw, mem.p, F);
        else smooth_work_carve(rw, mem.p, F);
        if (F > 1) {
            if ((rc = upload_lambda(sp))) return rc;
            if (cv) {
                std::vector<double> ratio((size_t)F, 0.0);
                auto dt = [&](int f) { return sp.frame_time ? sp.frame_time[f + 1] - sp.frame_time[f] : 1.0; };
                for (int f = 1; f + 1 < F; f++) ratio[f] = dt(f) / dt(f - 1);
                if ((rc = copy_h2d(pb, cw.ratio, ratio.data(), ratio.size() * sizeof(double)))) return rc;
            } else if (sp.rel_motion) {
                if ((rc = copy_h2d(pb, rw.rel_buf, sp.rel_motion, 6 * (size_t)(F - 1) * sizeof(double)))) return rc;
                rw.rel = rw.rel_buf;
            }
        }
        if (F) HIP_TRY(hipMemcpyAsync(z(0), P.z[pb->cur] + 6 * (size_t)P.A, 6 * (size_t)F * sizeof(double), hipMemcpyDeviceToDevice, pb->stream));
        return AAR_OK;
    }

    // H at z[cur] (mu = 0) with its costs into res(), the solve's elimination, then the selected inverse on area: selinv_doubles() zeroed
    // doubles of the caller's (F > 0).  Launches only.
    size_t selinv_doubles() const { return cv ? smooth_cv_selinv_doubles(pb->P.F) : 72 * (size_t)pb->P.F; }
    SmoothSel selinv(int cur, double *area) const {
        const int F = pb->P.F;
        SmoothSel s;
        eval(cur, /*with_j=*/true);
        s.launches = 2 + solve(0.0);
        if (cv) {
            s.launches += launch_smooth_cv_selinv(cw, F, area, &s.fc, &s.lc, &s.l2, pb->stream);
        } else {
            s.fc = area; s.lc = area + 36 * (size_t)F;
            s.launches += launch_smooth_selinv(rw, F, s.fc, s.lc, pb->stream);
        }
        return s;
    }

    // after selinv: the record (res [8], or NULL to leave it) and the elimination's pivot flag read back, and the refusal of a raised flag
    int read_pivot(const char *who, const char *kernels, double *res8) const {
        int rc = AAR_OK;
        int32_t f = 0;
        if (res8 && (rc = copy_d2h(pb, res8, res(), 8 * sizeof(double)))) return rc;
        if ((rc = copy_d2h(pb, &f, flag(), sizeof f))) return rc;
        if ((rc = check_async(kernels))) return rc;
        return f ? pivot_refusal(who) : AAR_OK;
    }
    int pivot_refusal(const char *who) const {
        return set_error(AAR_ERR_NUMERIC, "%s: non-positive pivot in the %s elimination (the frames' detections and the prior do not determine "
                                          "every pose)", who, elimination());
    }
};

// the head of the covariance, query and relative reports, and their tail: sigma2 over the degrees of freedom, the seconds since t0, and the
// copy bounded by the caller's struct_size
extern "C++" template <class R>
void smooth_report_begin(const aar_problem *pb, R &r) {
    memset(&r, 0, sizeof r);
    r.num_residuals = 8 * (int64_t)pb->P.N + 6 * (int64_t)std::max(pb->P.F - 1, 0);
    r.num_vars = 6 * (int64_t)pb->P.F;
}
extern "C++" template <class R>
void smooth_report_out(R &r, R *report, std::chrono::steady_clock::time_point t0) {
    r.seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    if (!report) return;
    r.struct_size = report->struct_size;
    memcpy(report, &r, std::min<size_t>(report->struct_size, sizeof r));
}
extern "C++" template <class R>
void smooth_report_end(R &r, R *report, std::chrono::steady_clock::time_point t0) {
    const int64_t dof = r.num_residuals - r.num_vars;
    r.sigma2 = dof > 0 ? (r.data_cost + r.prior_cost) / (double)dof : 0.0;
    smooth_report_out(r, report, t0);
}

// the entries whose selected inverse is the tridiagonal one
int smooth_rw_only(const aar_smooth_params &sp, const char *who) {
    if (sp.model == AAR_SMOOTH_MODEL_CONSTANT_VELOCITY)
        return set_error(AAR_ERR_UNSUPPORTED, "%s: model = AAR_SMOOTH_MODEL_CONSTANT_VELOCITY is not supported here (this entry works on the selected "
                                              "inverse of the block-tridiagonal system; the pose covariance under constant velocity is "
                                              "aar_track_smooth_covariance2, the sigma fit aar_track_smooth_fit2 and aar_track_smooth_fit_terms2, "
                                              "the track at any time aar_track_smooth_query2); "
                                              "use AAR_SMOOTH_MODEL_RANDOM_WALK", who);
    return AAR_OK;
}

// the checks every entry makes on its parameters; c: the record of the call, no device work yet
int smooth_entry(aar_problem *pb, const aar_smooth_params *sp_in, SmoothRun &c, const char *who) {
    if (!sp_in) return set_error(AAR_ERR_INVALID, "%s: null aar_smooth_params", who);
    int rc = aar_smooth_params_validate(pb->L.F, sp_in);
    if (rc) return rc;
    (void)smooth_params_read(sp_in, &c.sp);
    c.pb = pb;
    c.cv = c.sp.model == AAR_SMOOTH_MODEL_CONSTANT_VELOCITY;
    if (pb->comm) return set_error(AAR_ERR_UNSUPPORTED, "%s: the motion prior couples frames across shard boundaries; smoothed tracking is single-GPU only", who);
    return AAR_OK;
}

// what one run of the joint LM leaves on the host; cur: in = the buffer of c.z the run starts from, out = the one that holds its result
struct SmoothLm {
    int cur = 0, iters = 0, rejected = 0, mustExit = 0;
    double initial = 0.0, currErr = 0.0, currData = 0.0, currPrior = 0.0, mu = -1.0;
};

// aar_track_smooth's loop on a prepared record, from its z[s.cur]
int smooth_lm(const SmoothRun &o, const aar_lm_params &p, SmoothLm &s) {
    aar_problem *pb = o.pb;
    DeviceProblem &P = pb->P;
    const int F = P.F;
    const double rows = 8.0 * (double)P.N + 6.0 * (double)(F - 1);
    int rc = AAR_OK;
    int cur = s.cur, iters = 0, rejected = 0, mustExit = 0;
    double res[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    double currData = 0.0, currPrior = 0.0, mu = -1.0, v = 2.0;
    if (F > 0) {
        // init: the first evaluation also yields the first step's system
        o.eval(cur, true);
        pb->launches += 2;
        if ((rc = copy_d2h(pb, res, o.res(), sizeof res))) return rc;
        currData = res[0]; currPrior = res[1];
    }
    double currErr = currData + currPrior, prevErr = currErr;
    const double initial = currErr;
    for (int it = 0; it < p.max_iters && !mustExit && rows > 0 && F > 0; it++) {
        if (it > 0) { o.eval(cur, true); pb->launches += 2; }   // H, b at curr_z (its costs are those already held)
        if (mu < 0) mu = res[4] * p.tau;   // (first iteration: res still holds the initial evaluation's record)
        double gain = 0.0;
        int ntries = 0;
        bool accepted = false;
        do {
            pb->launches += o.solve(mu);
            o.eval(cur, false);   // z[1 - cur] = z[cur] + delta, its costs, |delta|^2, delta . b
            pb->launches += 2;
            if ((rc = copy_d2h(pb, res, o.res(), sizeof res))) return rc;   // the try's one read-back
            const double err = res[0] + res[1];
            const bool bad_pivot = res[5] != 0.0;
            const double Lq = 0.5 * (mu * res[2] - res[3]);
            gain = (err - prevErr) / Lq;
            if (!bad_pivot && gain > 0 && (err - prevErr) < 0) {
                const double t = 2 * gain - 1;
                mu = mu * std::max(0.33, 1.0 - t * t * t);
                v = 2.0;
                currErr = err; currData = res[0]; currPrior = res[1];
                cur = 1 - cur;
                accepted = true;
            } else {
                if (bad_pivot) gain = 0.0;   // a failed factorisation is a rejected try: more damping, and the retry rule below applies
                mu = mu * v;
                v = v * 5;
                rejected++;
            }
        } while (gain <= 0 && ntries++ < 5 && !accepted);
        if (currErr < p.min_error) mustExit = 1;
        if (std::fabs(prevErr - currErr) <= p.min_step_error_diff || std::fabs((prevErr - currErr) / rows) <= p.min_average_step_error_diff || !accepted)
            mustExit = 2;
        if (currErr > prevErr) mustExit = 3;
        iters++;
        prevErr = currErr;
    }
    s.cur = cur; s.iters = iters; s.rejected = rejected; s.mustExit = mustExit;
    s.initial = initial; s.currErr = currErr; s.currData = currData; s.currPrior = currPrior; s.mu = mu;
    return AAR_OK;
}

// the frame poses of the problem's pose vector into x_full
int smooth_download(aar_problem *pb, double *x_full) {
    // only the frame poses move; download_z honours the Config flags, so force "frames on, shared off" for this call
    PoseLayout keep = pb->L;
    pb->L.oc = false; pb->L.om = false; pb->L.of = true;
    int rc = download_z(pb, pb->cur, x_full);
    pb->L = keep;
    return rc;
}

}  // namespace

int32_t aar_smooth_solve_launches(int32_t num_frames, int32_t model) {
    const int F = num_frames;
    if (F <= 0) return 0;
    if (model == AAR_SMOOTH_MODEL_CONSTANT_VELOCITY) return smooth_cv_solve_launches(F);
    // smooth_kernels.hip: a level of its own while more than SMOOTH_TAIL nodes eliminate, with the damping in front and a back-substitution each
    int n = 0;
    for (int s = 1; s < F && (F + 2 * s - 1) / (2 * s) > SMOOTH_TAIL; s *= 2) n++;
    return n ? 2 * n + 2 : 1;
}

int aar_smooth_params_validate(int32_t num_frames, const aar_smooth_params *sp_in) {
    if (!sp_in) return set_error(AAR_ERR_INVALID, "aar_smooth_params_validate: null argument");
    if (num_frames < 0) return set_error(AAR_ERR_INVALID, "aar_smooth_params: num_frames %d is negative", (int)num_frames);
    aar_smooth_params sp;
    if (!smooth_params_read(sp_in, &sp))
        return set_error(AAR_ERR_INVALID, "aar_smooth_params: struct_size %u does not reach sigma_rot / sigma_trans", (unsigned)sp_in->struct_size);
    if (!(sp.sigma_rot > 0.0) || !std::isfinite(sp.sigma_rot)) return set_error(AAR_ERR_INVALID, "aar_smooth_params: sigma_rot = %g must be positive and finite", sp.sigma_rot);
    if (!(sp.sigma_trans > 0.0) || !std::isfinite(sp.sigma_trans)) return set_error(AAR_ERR_INVALID, "aar_smooth_params: sigma_trans = %g must be positive and finite", sp.sigma_trans);
    if (sp.model != AAR_SMOOTH_MODEL_RANDOM_WALK && sp.model != AAR_SMOOTH_MODEL_CONSTANT_VELOCITY)
        return set_error(AAR_ERR_INVALID, "aar_smooth_params: model = %d is neither AAR_SMOOTH_MODEL_RANDOM_WALK nor AAR_SMOOTH_MODEL_CONSTANT_VELOCITY", (int)sp.model);
    if (sp.model == AAR_SMOOTH_MODEL_CONSTANT_VELOCITY) {
        if (!(sp.sigma_rot0 > 0.0) || !std::isfinite(sp.sigma_rot0))
            return set_error(AAR_ERR_INVALID, "aar_smooth_params: sigma_rot0 = %g must be positive and finite under AAR_SMOOTH_MODEL_CONSTANT_VELOCITY", sp.sigma_rot0);
        if (!(sp.sigma_trans0 > 0.0) || !std::isfinite(sp.sigma_trans0))
            return set_error(AAR_ERR_INVALID, "aar_smooth_params: sigma_trans0 = %g must be positive and finite under AAR_SMOOTH_MODEL_CONSTANT_VELOCITY", sp.sigma_trans0);
        if (sp.rel_motion)
            return set_error(AAR_ERR_INVALID, "aar_smooth_params: rel_motion must be NULL under AAR_SMOOTH_MODEL_CONSTANT_VELOCITY (the expected motion "
                                              "of a term is the motion of the pair before it)");
    }
    if (sp.frame_time)
        for (int f = 0; f < num_frames; f++) {
            if (!std::isfinite(sp.frame_time[f])) return set_error(AAR_ERR_INVALID, "aar_smooth_params: frame_time[%d] is not finite", f);
            if (f > 0 && !(sp.frame_time[f] > sp.frame_time[f - 1]))
                return set_error(AAR_ERR_INVALID, "aar_smooth_params: frame_time[%d] = %g does not ascend from frame_time[%d] = %g", f, sp.frame_time[f], f - 1, sp.frame_time[f - 1]);
            if (f > 0 && !std::isfinite(sp.frame_time[f] - sp.frame_time[f - 1]))
                return set_error(AAR_ERR_INVALID, "aar_smooth_params: frame_time[%d] - frame_time[%d] overflows", f, f - 1);
        }
    if (sp.rel_motion)
        for (int f = 0; f + 1 < num_frames; f++)
            for (int k = 0; k < 6; k++)
                if (!std::isfinite(sp.rel_motion[6 * (size_t)f + k])) return set_error(AAR_ERR_INVALID, "aar_smooth_params: rel_motion[%d][%d] is not finite", f, k);
    return AAR_OK;
}

namespace {

// aar_track_smooth_system and aar_track_smooth_system2 after their checks; off2 is written under constant velocity only
int smooth_system(SmoothRun &c, const char *who, const double *x_full, double mu, double *diag, double *off, double *off2, double *rhs,
                  double *delta, double cost[2]) {
    aar_problem *pb = c.pb;
    const int F = pb->P.F;
    int rc = c.begin(x_full);
    if (rc) return rc;
    if (cost) cost[0] = cost[1] = 0.0;
    if (F == 0) { HIP_TRY(hipStreamSynchronize(pb->stream)); return AAR_OK; }
    c.eval(0, /*with_j=*/true);
    double res[8];
    if ((rc = copy_d2h(pb, res, c.res(), sizeof res))) return rc;
    if (cost) { cost[0] = res[0]; cost[1] = res[1]; }
    if (diag && (rc = copy_d2h(pb, diag, c.cv ? c.cw.Dg : c.rw.Dg, 36 * (size_t)F * sizeof(double)))) return rc;
    if (off && F > 1 && (rc = copy_d2h(pb, off, c.cv ? c.cw.O1 : c.rw.Of, 36 * (size_t)(F - 1) * sizeof(double)))) return rc;
    if (c.cv && off2 && F > 2 && (rc = copy_d2h(pb, off2, c.cw.O2, 36 * (size_t)(F - 2) * sizeof(double)))) return rc;
    if (rhs && (rc = copy_d2h(pb, rhs, c.cv ? c.cw.rhs : c.rw.rhs, 6 * (size_t)F * sizeof(double)))) return rc;
    if (delta) {
        pb->launches += c.solve(mu);
        int32_t flag = 0;
        if ((rc = copy_d2h(pb, &flag, c.flag(), sizeof flag))) return rc;
        if ((rc = copy_d2h(pb, delta, c.cv ? c.cw.delta : c.rw.delta, 6 * (size_t)F * sizeof(double)))) return rc;
        if (flag) return set_error(AAR_ERR_NUMERIC, "%s: non-positive pivot in the %s solve (mu = %g)", who, c.elimination(), mu);
    }
    return check_async("smoothing kernels");
}

// DESIGN.md sections 28 and 32: H at mu = 0 as smooth_system assembles it, the solve's elimination, then the downward pass of
// smooth_cov_kernels.hip or smooth_cv_cov_kernels.hip over what the elimination kept; lag2_cov under constant velocity only
int smooth_covariance(SmoothRun &c, const char *who, const double *x_full, double *frame_cov, double *lag_cov, double *lag2_cov,
                      aar_smooth_covariance_report *report) {
    aar_problem *pb = c.pb;
    const int F = pb->P.F;
    const auto t0 = std::chrono::steady_clock::now();
    int rc = c.begin(x_full);
    if (rc) return rc;
    aar_smooth_covariance_report r;
    smooth_report_begin(pb, r);
    if (F > 0) {
        // the selected inverse's area: an allocation of its own, the carve of the solve's work area keeps its layout
        DevMem area;
        if ((rc = area.alloc(pb, c.selinv_doubles()))) return rc;
        const SmoothSel sel = c.selinv(0, area.p);
        r.launches = sel.launches;
        pb->launches += r.launches;
        double res[8];
        if ((rc = c.read_pivot(who, "smoothing covariance kernels", res))) return rc;
        r.data_cost = res[0]; r.prior_cost = res[1];
        if (frame_cov && (rc = copy_d2h(pb, frame_cov, sel.fc, 36 * (size_t)F * sizeof(double)))) return rc;
        if (lag_cov && F > 1 && (rc = copy_d2h(pb, lag_cov, sel.lc, 36 * (size_t)(F - 1) * sizeof(double)))) return rc;
        if (lag2_cov && F > 2 && (rc = copy_d2h(pb, lag2_cov, sel.l2, 36 * (size_t)(F - 2) * sizeof(double)))) return rc;
    } else {
        HIP_TRY(hipStreamSynchronize(pb->stream));
    }
    smooth_report_end(r, report, t0);
    return AAR_OK;
}

}  // namespace

int aar_track_smooth_system(aar_problem *pb, const double *x_full, const aar_smooth_params *sp_in, double mu, double *diag, double *off, double *rhs,
                            double *delta, double cost[2]) {
    if (!pb || !x_full) return set_error(AAR_ERR_INVALID, "aar_track_smooth_system: null argument");
    if (!(mu >= 0.0) || !std::isfinite(mu)) return set_error(AAR_ERR_INVALID, "aar_track_smooth_system: mu = %g must be finite and not negative", mu);
    SmoothRun c;
    int rc = smooth_entry(pb, sp_in, c, "aar_track_smooth_system");
    if (rc) return rc;
    if (c.cv)
        return set_error(AAR_ERR_UNSUPPORTED, "aar_track_smooth_system: model = AAR_SMOOTH_MODEL_CONSTANT_VELOCITY has a second off-diagonal; "
                                              "call aar_track_smooth_system2");
    return smooth_system(c, "aar_track_smooth_system", x_full, mu, diag, off, nullptr, rhs, delta, cost);
}

// under the random walk aar_track_smooth_system itself (its name in the messages), and off2 zero
int aar_track_smooth_system2(aar_problem *pb, const double *x_full, const aar_smooth_params *sp_in, double mu, double *diag, double *off, double *off2,
                             double *rhs, double *delta, double cost[2]) {
    if (!pb || !x_full) return set_error(AAR_ERR_INVALID, "aar_track_smooth_system2: null argument");
    if (!(mu >= 0.0) || !std::isfinite(mu)) return set_error(AAR_ERR_INVALID, "aar_track_smooth_system2: mu = %g must be finite and not negative", mu);
    SmoothRun c;
    int rc = smooth_entry(pb, sp_in, c, "aar_track_smooth_system2");
    if (rc) return rc;
    if ((rc = smooth_system(c, c.cv ? "aar_track_smooth_system2" : "aar_track_smooth_system", x_full, mu, diag, off, off2, rhs, delta, cost))) return rc;
    if (!c.cv && off2 && pb->P.F > 2) std::fill(off2, off2 + 36 * (size_t)(pb->P.F - 2), 0.0);
    return AAR_OK;
}

int aar_track_smooth_covariance(aar_problem *pb, const double *x_full, const aar_smooth_params *sp_in, double *frame_cov, double *lag_cov,
                                aar_smooth_covariance_report *report) {
    if (!pb || !x_full) return set_error(AAR_ERR_INVALID, "aar_track_smooth_covariance: null argument");
    SmoothRun c;
    int rc = smooth_entry(pb, sp_in, c, "aar_track_smooth_covariance");
    if (rc) return rc;
    if ((rc = smooth_rw_only(c.sp, "aar_track_smooth_covariance"))) return rc;
    return smooth_covariance(c, "aar_track_smooth_covariance", x_full, frame_cov, lag_cov, nullptr, report);
}

// under the random walk aar_track_smooth_covariance itself (its name in the messages)
int aar_track_smooth_covariance2(aar_problem *pb, const double *x_full, const aar_smooth_params *sp_in, double *frame_cov, double *lag_cov,
                                 double *lag2_cov, aar_smooth_covariance_report *report) {
    if (!pb || !x_full) return set_error(AAR_ERR_INVALID, "aar_track_smooth_covariance2: null argument");
    SmoothRun c;
    int rc = smooth_entry(pb, sp_in, c, "aar_track_smooth_covariance2");
    if (rc) return rc;
    if (!c.cv && lag2_cov)
        return set_error(AAR_ERR_UNSUPPORTED, "aar_track_smooth_covariance2: lag2_cov under AAR_SMOOTH_MODEL_RANDOM_WALK is not supported (the "
                                              "selected inverse of the block-tridiagonal system does not contain the lag-two blocks)");
    return smooth_covariance(c, c.cv ? "aar_track_smooth_covariance2" : "aar_track_smooth_covariance", x_full, frame_cov, lag_cov, lag2_cov, report);
}

int aar_track_smooth(aar_problem *pb, double *x_full, const aar_lm_params *prm, const aar_smooth_params *sp_in, double *frame_err, double *pair_err,
                     aar_smooth_report *report) {
    if (!pb || !x_full) return set_error(AAR_ERR_INVALID, "aar_track_smooth: null argument");
    SmoothRun c;
    int rc = smooth_entry(pb, sp_in, c, "aar_track_smooth");
    if (rc) return rc;
    DeviceProblem &P = pb->P;
    aar_lm_params p;
    if (prm) p = *prm; else aar_lm_default_params(&p);
    const int F = P.F;
    const auto t0 = std::chrono::steady_clock::now();
    if ((rc = c.begin(x_full))) return rc;
    SmoothLm s;
    if ((rc = smooth_lm(c, p, s))) return rc;
    if (F) HIP_TRY(hipMemcpyAsync(P.z[pb->cur] + 6 * (size_t)P.A, c.z(s.cur), 6 * (size_t)F * sizeof(double), hipMemcpyDeviceToDevice, pb->stream));
    if (frame_err && F && (rc = copy_d2h(pb, frame_err, c.Ef(s.cur), (size_t)F * sizeof(double)))) return rc;
    if (pair_err && F > 1 && (rc = copy_d2h(pb, pair_err, c.Pe(s.cur), (size_t)(F - 1) * sizeof(double)))) return rc;
    if ((rc = check_async("smoothing kernels"))) return rc;
    if ((rc = smooth_download(pb, x_full))) return rc;
    if (report) {
        aar_smooth_report r;
        memset(&r, 0, sizeof r);
        r.iterations = s.iters; r.stop_code = s.mustExit; r.rejected_tries = s.rejected;
        r.initial_cost = s.initial; r.final_cost = s.currErr; r.final_data_cost = s.currData; r.final_prior_cost = s.currPrior;
        r.final_mu = s.mu;
        smooth_report_out(r, report, t0);
    }
    return AAR_OK;
}

// ------------------------------------------------------------------------------------------------
// Fitting the smoother's noise levels (DESIGN.md sections 29 and 33, smooth_fit_kernels.hip and smooth_cv_fit_kernels.hip)
// ------------------------------------------------------------------------------------------------
namespace {

// the caller's struct read up to its struct_size, the rest at the defaults; false: too short to hold struct_size itself
bool smooth_fit_params_read(const aar_smooth_fit_params *in, aar_smooth_fit_params *out) {
    aar_smooth_fit_default_params(out);
    if (in->struct_size < sizeof(uint32_t)) return false;
    memcpy(out, in, std::min<size_t>(in->struct_size, sizeof *out));
    out->struct_size = (uint32_t)sizeof *out;
    return true;
}

// what the fit entries refuse, after smooth_entry and before anything is sized by F - 1
int smooth_fit_entry(const SmoothRun &c, const char *who) {
    const aar_problem *pb = c.pb;
    if (pb->with_huber)
        return set_error(AAR_ERR_UNSUPPORTED, "%s: the problem was created with_huber; the Huber weights break the Gaussian data model the fit "
                                              "rests on", who);
    if (!c.cv && pb->L.F < 2) return set_error(AAR_ERR_INVALID, "%s: num_frames = %d, the fit needs at least one pair of frames", who, (int)pb->L.F);
    if (c.cv && pb->L.F < 3)
        return set_error(AAR_ERR_INVALID, "%s: num_frames = %d, the fit under AAR_SMOOTH_MODEL_CONSTANT_VELOCITY needs at least one "
                                          "second-difference term (three frames)", who, (int)pb->L.F);
    if (pb->P.N < 1) return set_error(AAR_ERR_INVALID, "%s: the problem has no detections", who);
    return AAR_OK;
}

// the selected inverse's area, the terms [F-1][4] and the record the host reads: one allocation
struct SmoothFitBuf {
    DevMem mem;
    double *terms = nullptr, *rec = nullptr;
    int alloc(const SmoothRun &c) {
        const size_t F = (size_t)c.pb->P.F, na = c.selinv_doubles();
        int rc = mem.alloc(c.pb, na + 4 * (F - 1) + 8);
        terms = mem.p + na; rec = terms + 4 * (F - 1);
        return rc;
    }
};

// the E-step at c.z(cur) with the lambda on the device (built with eff's sigmas): launches, then the one read-back of rec [8] = A_r, U_r,
// A_t, U_t (under constant velocity over the terms 1 .. F-2), data cost, prior cost, pivot flag, and u_0 of pair 0 (zero under the random walk)
int smooth_fit_estep(const SmoothRun &c, int cur, const aar_smooth_params &eff, const SmoothFitBuf &b, double rec[8], const char *who) {
    aar_problem *pb = c.pb;
    const int F = pb->P.F;
    const SmoothSel sel = c.selinv(cur, b.mem.p);
    int launches = sel.launches;
    if (c.cv)
        launches += launch_smooth_cv_fit_terms(c.cw, cur, F, eff.sigma_rot, eff.sigma_rot0, eff.sigma_trans0, sel.fc, sel.lc, sel.l2, b.terms, b.rec,
                                               pb->stream);
    else launches += launch_smooth_fit_terms(c.rw, cur, F, eff.sigma_rot, sel.fc, sel.lc, b.terms, b.rec, pb->stream);
    pb->launches += launches;
    int rc = copy_d2h(pb, rec, b.rec, 8 * sizeof(double));
    if (rc) return rc;
    return rec[6] != 0.0 ? c.pivot_refusal(who) : AAR_OK;
}

// aar_track_smooth_fit_terms and aar_track_smooth_fit_terms2 after their model checks; six: sums holds u_0 and pair 0's cost as well
int smooth_fit_terms(SmoothRun &c, const char *who, const double *x_full, double *pair_terms, double *sums, bool six) {
    aar_problem *pb = c.pb;
    int rc = smooth_fit_entry(c, who);
    if (rc) return rc;
    if ((rc = c.begin(x_full))) return rc;
    SmoothFitBuf b;
    if ((rc = b.alloc(c))) return rc;
    double rec[8], pair0 = 0.0;
    if ((rc = smooth_fit_estep(c, 0, c.sp, b, rec, who))) return rc;
    if (c.cv && (rc = copy_d2h(pb, &pair0, c.Pe(0), sizeof pair0))) return rc;   // the evaluation's cost of pair 0
    if (pair_terms && (rc = copy_d2h(pb, pair_terms, b.terms, 4 * (size_t)(pb->P.F - 1) * sizeof(double)))) return rc;
    if ((rc = check_async("smoothing fit kernels"))) return rc;
    if (sums) for (int i = 0; i < 4; i++) sums[i] = rec[i];
    if (sums && six) { sums[4] = c.cv ? rec[7] : 0.0; sums[5] = pair0; }
    return AAR_OK;
}

// aar_track_smooth_fit and aar_track_smooth_fit2 after their model checks: EM over q = sigma_px^2 and the physical variances s_r, s_t of the
// pairs (random walk) or of the terms 1 .. F-2 (constant velocity, pair 0's sigmas physical and held); the smoother runs at sigma / sqrt(q)
int smooth_fit(SmoothRun &c, const char *who, double *x_full, const aar_lm_params *prm, const aar_smooth_fit_params *fp_in, double *path,
               aar_smooth_fit_report *report) {
    aar_problem *pb = c.pb;
    const aar_smooth_params &sp = c.sp;
    aar_smooth_fit_params fp;
    int rc = AAR_OK;
    if (fp_in) {
        if ((rc = aar_smooth_fit_params_validate(fp_in))) return rc;
        (void)smooth_fit_params_read(fp_in, &fp);
    } else {
        aar_smooth_fit_default_params(&fp);
    }
    if ((rc = smooth_fit_entry(c, who))) return rc;
    DeviceProblem &P = pb->P;
    aar_lm_params p;
    if (prm) p = *prm; else aar_lm_default_params(&p);
    const int F = P.F;
    const auto t0 = std::chrono::steady_clock::now();
    const int64_t launches0 = pb->launches;
    if ((rc = c.begin(x_full))) return rc;   // lambda at the start values, the ratios once
    SmoothFitBuf b;
    if ((rc = b.alloc(c))) return rc;
    double q = 1.0, s_r = sp.sigma_rot * sp.sigma_rot, s_t = sp.sigma_trans * sp.sigma_trans;
    aar_smooth_fit_report r;
    memset(&r, 0, sizeof r);
    std::vector<double> rows;   // the path, handed over only when the fit has succeeded
    rows.insert(rows.end(), {1.0, sp.sigma_rot, sp.sigma_trans});
    aar_smooth_params eff = sp;   // frame_time and rel_motion kept, the sigmas replaced
    SmoothLm s;
    const double terms_n = 3.0 * (double)(c.cv ? F - 2 : F - 1);
    double rec[8] = {0, 0, 0, 0, 0, 0, 0, 0}, u_d = 0.0;
    r.stop_code = 2;
    for (int it = 0; it < fp.max_iters; it++) {
        if (it > 0 && (rc = c.upload_lambda(eff))) return rc;
        if ((rc = smooth_lm(c, p, s))) return rc;
        r.lm_steps += s.iters;
        if ((rc = smooth_fit_estep(c, s.cur, eff, b, rec, who))) return rc;
        const double er2 = eff.sigma_rot * eff.sigma_rot, et2 = eff.sigma_trans * eff.sigma_trans;
        u_d = 6.0 * (double)F - rec[1] / er2 - rec[3] / et2;
        if (c.cv) u_d -= rec[7];
        const double n_r = fp.estimate_rot ? (rec[0] + q * rec[1]) / terms_n : s_r;
        const double n_t = fp.estimate_trans ? (rec[2] + q * rec[3]) / terms_n : s_t;
        const double n_q = fp.estimate_px ? (rec[4] + q * u_d) / (8.0 * (double)P.N) : q;
        const double was[3] = {q, s_r, s_t}, now[3] = {n_q, n_r, n_t};
        const char *names[3] = {"sigma_px", "sigma_rot", "sigma_trans"};
        double change = 0.0;
        for (int i = 0; i < 3; i++) {
            if (!(now[i] > 0.0) || !std::isfinite(now[i]))
                return set_error(AAR_ERR_NUMERIC, "%s: iteration %d: the M-step gives the variance %g for %s", who, it + 1, now[i], names[i]);
            change = std::max(change, std::fabs(std::sqrt(now[i]) - std::sqrt(was[i])) / std::sqrt(was[i]));
        }
        q = n_q; s_r = n_r; s_t = n_t;
        const double sq = std::sqrt(q);
        eff.sigma_rot = std::sqrt(s_r / q);
        eff.sigma_trans = std::sqrt(s_t / q);
        if (c.cv) { eff.sigma_rot0 = sp.sigma_rot0 / sq; eff.sigma_trans0 = sp.sigma_trans0 / sq; }
        r.iterations = it + 1;
        r.last_rel_change = change;
        rows.insert(rows.end(), {sq, std::sqrt(s_r), std::sqrt(s_t)});
        if (change < fp.rel_tol) { r.stop_code = 1; break; }
    }
    // the track at the fitted values
    if ((rc = c.upload_lambda(eff))) return rc;
    if ((rc = smooth_lm(c, p, s))) return rc;
    r.lm_steps += s.iters;
    HIP_TRY(hipMemcpyAsync(P.z[pb->cur] + 6 * (size_t)P.A, c.z(s.cur), 6 * (size_t)F * sizeof(double), hipMemcpyDeviceToDevice, pb->stream));
    if ((rc = check_async("smoothing fit kernels"))) return rc;
    if ((rc = smooth_download(pb, x_full))) return rc;
    if (path) std::copy(rows.begin(), rows.end(), path);
    if (report) {
        r.sigma_px = std::sqrt(q); r.sigma_rot = std::sqrt(s_r); r.sigma_trans = std::sqrt(s_t);
        r.sigma_rot_eff = eff.sigma_rot; r.sigma_trans_eff = eff.sigma_trans;
        r.launches = (int32_t)(pb->launches - launches0);
        r.a_rot = rec[0]; r.u_rot = rec[1]; r.a_trans = rec[2]; r.u_trans = rec[3]; r.u_data = u_d; r.data_cost = rec[4];
        smooth_report_out(r, report, t0);
    }
    return AAR_OK;
}

}  // namespace

void aar_smooth_fit_default_params(aar_smooth_fit_params *p) {
    if (!p) return;
    memset(p, 0, sizeof *p);
    p->struct_size = (uint32_t)sizeof *p;
    p->max_iters = 50;
    p->rel_tol = 1e-3;
    p->estimate_px = p->estimate_rot = p->estimate_trans = 1;
}

int aar_smooth_fit_params_validate(const aar_smooth_fit_params *in) {
    if (!in) return set_error(AAR_ERR_INVALID, "aar_smooth_fit_params_validate: null argument");
    aar_smooth_fit_params p;
    if (!smooth_fit_params_read(in, &p))
        return set_error(AAR_ERR_INVALID, "aar_smooth_fit_params: struct_size %u does not reach past struct_size itself", (unsigned)in->struct_size);
    if (p.max_iters < 1) return set_error(AAR_ERR_INVALID, "aar_smooth_fit_params: max_iters = %d must be at least 1", (int)p.max_iters);
    if (!(p.rel_tol >= 0.0) || !std::isfinite(p.rel_tol))
        return set_error(AAR_ERR_INVALID, "aar_smooth_fit_params: rel_tol = %g must be finite and not negative", p.rel_tol);
    const int32_t est[3] = {p.estimate_px, p.estimate_rot, p.estimate_trans};
    const char *names[3] = {"estimate_px", "estimate_rot", "estimate_trans"};
    for (int i = 0; i < 3; i++)
        if (est[i] != 0 && est[i] != 1) return set_error(AAR_ERR_INVALID, "aar_smooth_fit_params: %s = %d must be 0 or 1", names[i], (int)est[i]);
    if (!p.estimate_px && !p.estimate_rot && !p.estimate_trans)
        return set_error(AAR_ERR_INVALID, "aar_smooth_fit_params: estimate_px, estimate_rot and estimate_trans are all 0, nothing to fit");
    return AAR_OK;
}

int aar_track_smooth_fit_terms(aar_problem *pb, const double *x_full, const aar_smooth_params *sp_in, double *pair_terms, double sums[4]) {
    if (!pb || !x_full) return set_error(AAR_ERR_INVALID, "aar_track_smooth_fit_terms: null argument");
    SmoothRun c;
    int rc = smooth_entry(pb, sp_in, c, "aar_track_smooth_fit_terms");
    if (rc) return rc;
    if ((rc = smooth_rw_only(c.sp, "aar_track_smooth_fit_terms"))) return rc;
    return smooth_fit_terms(c, "aar_track_smooth_fit_terms", x_full, pair_terms, sums, /*six=*/false);
}

// the ...2 entries: under the random walk the entry above itself (its name in the messages)
int aar_track_smooth_fit_terms2(aar_problem *pb, const double *x_full, const aar_smooth_params *sp_in, double *pair_terms, double sums[6]) {
    if (!pb || !x_full) return set_error(AAR_ERR_INVALID, "aar_track_smooth_fit_terms2: null argument");
    SmoothRun c;
    int rc = smooth_entry(pb, sp_in, c, "aar_track_smooth_fit_terms2");
    if (rc) return rc;
    return smooth_fit_terms(c, c.cv ? "aar_track_smooth_fit_terms2" : "aar_track_smooth_fit_terms", x_full, pair_terms, sums, /*six=*/true);
}

int aar_track_smooth_fit(aar_problem *pb, double *x_full, const aar_lm_params *prm, const aar_smooth_params *sp_in, const aar_smooth_fit_params *fp_in,
                         double *path, aar_smooth_fit_report *report) {
    if (!pb || !x_full) return set_error(AAR_ERR_INVALID, "aar_track_smooth_fit: null argument");
    SmoothRun c;
    int rc = smooth_entry(pb, sp_in, c, "aar_track_smooth_fit");
    if (rc) return rc;
    if ((rc = smooth_rw_only(c.sp, "aar_track_smooth_fit"))) return rc;
    return smooth_fit(c, "aar_track_smooth_fit", x_full, prm, fp_in, path, report);
}

int aar_track_smooth_fit2(aar_problem *pb, double *x_full, const aar_lm_params *prm, const aar_smooth_params *sp_in, const aar_smooth_fit_params *fp_in,
                          double *path, aar_smooth_fit_report *report) {
    if (!pb || !x_full) return set_error(AAR_ERR_INVALID, "aar_track_smooth_fit2: null argument");
    SmoothRun c;
    int rc = smooth_entry(pb, sp_in, c, "aar_track_smooth_fit2");
    if (rc) return rc;
    return smooth_fit(c, c.cv ? "aar_track_smooth_fit2" : "aar_track_smooth_fit", x_full, prm, fp_in, path, report);
}

// ------------------------------------------------------------------------------------------------
// The smoothed track at any time (smooth_query_kernels.hip)
// ------------------------------------------------------------------------------------------------
int aar_smooth_query_validate(int32_t num_frames, const aar_smooth_params *sp_in, int64_t n_query, const double *query_time) {
    if (!sp_in) return set_error(AAR_ERR_INVALID, "aar_smooth_query_validate: null aar_smooth_params");
    int rc = aar_smooth_params_validate(num_frames, sp_in);
    if (rc) return rc;
    if (n_query < 0 || n_query > INT32_MAX)
        return set_error(AAR_ERR_INVALID, "aar_smooth_query: n_query = %lld must lie in 0 .. %d", (long long)n_query, (int)INT32_MAX);
    if (n_query > 0 && !query_time) return set_error(AAR_ERR_INVALID, "aar_smooth_query: query_time is NULL with n_query = %lld", (long long)n_query);
    if (n_query > 0 && num_frames < 1)
        return set_error(AAR_ERR_INVALID, "aar_smooth_query: num_frames = %d, a query needs at least one frame", (int)num_frames);
    for (int64_t i = 0; i < n_query; i++)
        if (!std::isfinite(query_time[i])) return set_error(AAR_ERR_INVALID, "aar_smooth_query: query_time[%lld] is not finite", (long long)i);
    return AAR_OK;
}

namespace {

// the frame times as the device searches them, and the report's three counts from the same search on the host
void smooth_query_times(const aar_smooth_params &sp, int F, size_t Q, const double *query_time, std::vector<double> &ft, aar_smooth_query_report &r) {
    ft.resize((size_t)F);
    for (int f = 0; f < F; f++) ft[f] = sp.frame_time ? sp.frame_time[f] : (double)f;
    for (size_t i = 0; i < Q; i++) {
        const int s = (int)(std::upper_bound(ft.begin(), ft.end(), query_time[i]) - ft.begin()) - 1;
        if (s >= 0 && ft[s] == query_time[i]) r.num_on_frame++;
        else if (s < 0 || s == F - 1) r.num_outside++;
        else r.num_inside++;
    }
}

// What a time query leaves on the device: the poses, the blocks and the segments of Q > 0 times, in one allocation
struct SmoothQueryDev {
    DevMem out;
    double *pose = nullptr, *start = nullptr, *step = nullptr, *cov = nullptr;   // [Q][6] (start, step: constant velocity), [Q][36] or NULL
    int32_t *seg = nullptr, *flag = nullptr;   // [Q]; two pivot flags: the lag-three blocks', the queries'
    bool blocks = false;                       // the selected inverse ran
    int launches = 0;
};

// The device work of the query entries.  Random walk: the pose is a closed form of the frame poses, the selected inverse runs for cov alone.
// Constant velocity: H at mu = 0, its reduction and selected inverse, the lag-three blocks, then the queries; the pose depends on the
// blocks, so want_cov = false saves the blocks of the queries alone.  Launches and copies in, nothing read back
int smooth_query_device(SmoothRun &c, const double *x_full, size_t Q, const double *query_time, const std::vector<double> &ft, bool want_cov,
                        SmoothQueryDev &d) {
    aar_problem *pb = c.pb;
    const aar_smooth_params &sp = c.sp;
    DeviceProblem &P = pb->P;
    const int F = P.F;
    int rc;
    d.blocks = c.cv || want_cov;
    if ((rc = c.begin(x_full, d.blocks))) return rc;
    // one allocation: ft [F] | query times [Q] | pose [Q][6] | start, step [Q][6] each (constant velocity) | cov [Q][36] | the selected
    // inverse's area | l3 [F-3][36] (constant velocity) | segment [Q] and two pivot flags: the lag-three blocks', the queries'
    const size_t n_out = c.cv ? 18 * Q : 6 * Q, n_cov = want_cov ? 36 * Q : 0, n_sel = d.blocks ? c.selinv_doubles() : 0;
    const size_t n_dbl = (size_t)F + Q + n_out + n_cov + n_sel + (c.cv ? 36 * (size_t)std::max(F - 3, 0) : 0);
    if ((rc = d.out.alloc(pb, n_dbl, Q + 2))) return rc;
    double *d_ft = d.out.p, *d_qt = d_ft + F;
    d.pose = d_qt + Q; d.start = c.cv ? d.pose + 6 * Q : nullptr; d.step = c.cv ? d.start + 6 * Q : nullptr;
    d.cov = want_cov ? d.pose + n_out : nullptr;
    double *d_area = d.pose + n_out + n_cov, *d_l3 = d_area + n_sel;
    d.seg = reinterpret_cast<int32_t *>(d.out.p + n_dbl); d.flag = d.seg + Q;
    if ((rc = copy_h2d(pb, d_ft, ft.data(), (size_t)F * sizeof(double)))) return rc;
    if ((rc = copy_h2d(pb, d_qt, query_time, Q * sizeof(double)))) return rc;
    SmoothSel sel;
    if (d.blocks) sel = c.selinv(0, d_area);
    d.launches = sel.launches;
    if (c.cv) {
        d.launches += launch_smooth_cv_lag3(F, d_area, d_l3, d.flag, pb->stream);
        d.launches += launch_smooth_cv_query(F, c.z(0), d_ft, sp.sigma_rot, sp.sigma_trans, sp.sigma_rot0, sp.sigma_trans0, sel.fc, sel.lc, sel.l2,
                                             d_l3, (int64_t)Q, d_qt, d.pose, d.cov, d.start, d.step, d.seg, d.flag + 1, pb->stream);
    } else {
        d.launches += launch_smooth_query(c.rw, F, d.blocks ? c.z(0) : P.z[pb->cur] + 6 * (size_t)P.A, d_ft, sp.sigma_rot, sp.sigma_trans, sel.fc,
                                          sel.lc, (int64_t)Q, d_qt, d.pose, d.cov, d.seg, d.flag + 1, pb->stream);
    }
    return AAR_OK;
}

// ... and what is read back first: the chain's record and the three pivot flags, each with its refusal (d.blocks only)
int smooth_query_pivots(const SmoothRun &c, const char *who, const SmoothQueryDev &d, double res[8]) {
    int rc;
    int32_t qflag[2] = {0, 0};
    if ((rc = c.read_pivot(who, "smoothing query kernels", res))) return rc;
    if ((rc = copy_d2h(c.pb, qflag, d.flag, sizeof qflag))) return rc;
    if (qflag[0]) return set_error(AAR_ERR_NUMERIC, "%s: non-positive pivot in a supernode block of the lag-three blocks", who);
    if (qflag[1]) return set_error(AAR_ERR_NUMERIC, "%s: non-positive pivot in a query's %s", who, c.cv ? "eliminations" : "6x6 inverses");
    return AAR_OK;
}

// The three query entries after their model checks.  start, step: the start poses and delta_m (constant velocity, checking)
int smooth_query(SmoothRun &c, const char *who, const double *x_full, const aar_smooth_params *sp_in, int64_t n_query, const double *query_time,
                 double *pose, double *cov, int32_t *segment, double *start, double *step, aar_smooth_query_report *report) {
    aar_problem *pb = c.pb;
    const aar_smooth_params &sp = c.sp;
    int rc = aar_smooth_query_validate(pb->L.F, sp_in, n_query, query_time);
    if (rc) return rc;
    if (sp.rel_motion)
        return set_error(AAR_ERR_UNSUPPORTED, "%s: rel_motion is set; under an expected motion the pose of an inserted frame "
                                              "has no closed form (the split of dR does not commute)", who);
    const size_t Q = (size_t)n_query;
    const auto t0 = std::chrono::steady_clock::now();
    aar_smooth_query_report r;
    smooth_report_begin(pb, r);
    r.num_queries = (int32_t)Q;
    if (Q > 0) {
        std::vector<double> ft;
        smooth_query_times(sp, pb->P.F, Q, query_time, ft, r);
        SmoothQueryDev d;
        if ((rc = smooth_query_device(c, x_full, Q, query_time, ft, cov != nullptr, d))) return rc;
        r.launches = d.launches;
        pb->launches += r.launches;
        if (d.blocks) {
            double res[8];
            if ((rc = smooth_query_pivots(c, who, d, res))) return rc;
            r.data_cost = res[0]; r.prior_cost = res[1];
            if (cov && (rc = copy_d2h(pb, cov, d.cov, 36 * Q * sizeof(double)))) return rc;
        }
        if (pose && (rc = copy_d2h(pb, pose, d.pose, 6 * Q * sizeof(double)))) return rc;
        if (start && c.cv && (rc = copy_d2h(pb, start, d.start, 6 * Q * sizeof(double)))) return rc;
        if (step && c.cv && (rc = copy_d2h(pb, step, d.step, 6 * Q * sizeof(double)))) return rc;
        if (segment && (rc = copy_d2h(pb, segment, d.seg, Q * sizeof(int32_t)))) return rc;
        if ((rc = check_async("smoothing query kernels"))) return rc;
        HIP_TRY(hipStreamSynchronize(pb->stream));
    }
    smooth_report_end(r, report, t0);
    return AAR_OK;
}

}  // namespace

int aar_track_smooth_query(aar_problem *pb, const double *x_full, const aar_smooth_params *sp_in, int64_t n_query, const double *query_time,
                           double *pose, double *cov, int32_t *segment, aar_smooth_query_report *report) {
    if (!pb || !x_full) return set_error(AAR_ERR_INVALID, "aar_track_smooth_query: null argument");
    SmoothRun c;
    int rc = smooth_entry(pb, sp_in, c, "aar_track_smooth_query");
    if (rc) return rc;
    if ((rc = smooth_rw_only(c.sp, "aar_track_smooth_query"))) return rc;
    return smooth_query(c, "aar_track_smooth_query", x_full, sp_in, n_query, query_time, pose, cov, segment, nullptr, nullptr, report);
}

// under the random walk aar_track_smooth_query itself (its name in the messages)
int aar_track_smooth_query2(aar_problem *pb, const double *x_full, const aar_smooth_params *sp_in, int64_t n_query, const double *query_time,
                            double *pose, double *cov, int32_t *segment, aar_smooth_query_report *report) {
    if (!pb || !x_full) return set_error(AAR_ERR_INVALID, "aar_track_smooth_query2: null argument");
    SmoothRun c;
    int rc = smooth_entry(pb, sp_in, c, "aar_track_smooth_query2");
    if (rc) return rc;
    return smooth_query(c, c.cv ? "aar_track_smooth_query2" : "aar_track_smooth_query", x_full, sp_in, n_query, query_time, pose, cov, segment, nullptr,
                        nullptr, report);
}

int aar_track_smooth_query2_step(aar_problem *pb, const double *x_full, const aar_smooth_params *sp_in, int64_t n_query, const double *query_time,
                                 double *start_pose, double *step) {
    if (!pb || !x_full) return set_error(AAR_ERR_INVALID, "aar_track_smooth_query2_step: null argument");
    SmoothRun c;
    int rc = smooth_entry(pb, sp_in, c, "aar_track_smooth_query2_step");
    if (rc) return rc;
    if (!c.cv)
        return set_error(AAR_ERR_UNSUPPORTED, "aar_track_smooth_query2_step: model = AAR_SMOOTH_MODEL_RANDOM_WALK has no step (the pose of "
                                              "aar_track_smooth_query is a closed form); use AAR_SMOOTH_MODEL_CONSTANT_VELOCITY");
    return smooth_query(c, "aar_track_smooth_query2_step", x_full, sp_in, n_query, query_time, nullptr, nullptr, nullptr, start_pose, step, nullptr);
}

int aar_track_smooth_lag3(aar_problem *pb, const double *x_full, const aar_smooth_params *sp_in, double *lag3_cov) {
    if (!pb || !x_full) return set_error(AAR_ERR_INVALID, "aar_track_smooth_lag3: null argument");
    SmoothRun c;
    int rc = smooth_entry(pb, sp_in, c, "aar_track_smooth_lag3");
    if (rc) return rc;
    if (!c.cv)
        return set_error(AAR_ERR_UNSUPPORTED, "aar_track_smooth_lag3: model = AAR_SMOOTH_MODEL_RANDOM_WALK is not supported (the lag-three blocks "
                                              "belong to the selected inverse on supernodes of the block-pentadiagonal system); use "
                                              "AAR_SMOOTH_MODEL_CONSTANT_VELOCITY");
    const int F = pb->P.F;
    if (F < 4) return AAR_OK;
    if ((rc = c.begin(x_full))) return rc;
    // one allocation: the selected inverse's area | l3 [F-3][36] | the lag-three blocks' pivot flag
    const size_t na = c.selinv_doubles(), n3 = 36 * (size_t)(F - 3);
    DevMem sel;
    if ((rc = sel.alloc(pb, na + n3, 2))) return rc;
    double *d_l3 = sel.p + na;
    int32_t *d_flag = reinterpret_cast<int32_t *>(d_l3 + n3);
    pb->launches += c.selinv(0, sel.p).launches;
    pb->launches += launch_smooth_cv_lag3(F, sel.p, d_l3, d_flag, pb->stream);
    int32_t f3 = 0;
    if ((rc = c.read_pivot("aar_track_smooth_lag3", "smoothing query kernels", nullptr))) return rc;
    if ((rc = copy_d2h(pb, &f3, d_flag, sizeof f3))) return rc;
    if (f3) return set_error(AAR_ERR_NUMERIC, "aar_track_smooth_lag3: non-positive pivot in a supernode block of the lag-three blocks");
    if (lag3_cov && (rc = copy_d2h(pb, lag3_cov, d_l3, n3 * sizeof(double)))) return rc;
    return check_async("smoothing query kernels");
}

// ------------------------------------------------------------------------------------------------
// Covariance between any two frames, relative motion (smooth_relative_kernels.hip)
// ------------------------------------------------------------------------------------------------
int aar_smooth_relative_validate(int32_t num_frames, const aar_smooth_params *sp_in, int64_t n_pairs, const int32_t *frame_a, const int32_t *frame_b) {
    if (!sp_in) return set_error(AAR_ERR_INVALID, "aar_smooth_relative_validate: null aar_smooth_params");
    int rc = aar_smooth_params_validate(num_frames, sp_in);
    if (rc) return rc;
    if (n_pairs < 0 || n_pairs > INT32_MAX)
        return set_error(AAR_ERR_INVALID, "aar_smooth_relative: n_pairs = %lld must lie in 0 .. %d", (long long)n_pairs, (int)INT32_MAX);
    if (n_pairs > 0 && !frame_a) return set_error(AAR_ERR_INVALID, "aar_smooth_relative: frame_a is NULL with n_pairs = %lld", (long long)n_pairs);
    if (n_pairs > 0 && !frame_b) return set_error(AAR_ERR_INVALID, "aar_smooth_relative: frame_b is NULL with n_pairs = %lld", (long long)n_pairs);
    for (int64_t i = 0; i < n_pairs; i++) {
        if (frame_a[i] < 0 || frame_a[i] >= num_frames)
            return set_error(AAR_ERR_INVALID, "aar_smooth_relative: frame_a[%lld] = %d lies outside 0 .. num_frames - 1 = %d", (long long)i,
                             (int)frame_a[i], (int)num_frames - 1);
        if (frame_b[i] < 0 || frame_b[i] >= num_frames)
            return set_error(AAR_ERR_INVALID, "aar_smooth_relative: frame_b[%lld] = %d lies outside 0 .. num_frames - 1 = %d", (long long)i,
                             (int)frame_b[i], (int)num_frames - 1);
    }
    return AAR_OK;
}

int aar_track_smooth_relative(aar_problem *pb, const double *x_full, const aar_smooth_params *sp_in, int64_t n_pairs, const int32_t *frame_a,
                              const int32_t *frame_b, double *cross_cov, double *rel, double *rel_cov, aar_smooth_relative_report *report) {
    const char *who = "aar_track_smooth_relative";
    if (!pb || !x_full) return set_error(AAR_ERR_INVALID, "%s: null argument", who);
    SmoothRun c;
    int rc = smooth_entry(pb, sp_in, c, who);
    if (rc) return rc;
    if ((rc = aar_smooth_relative_validate(pb->L.F, sp_in, n_pairs, frame_a, frame_b))) return rc;
    const int F = pb->P.F;
    const size_t Q = (size_t)n_pairs;
    const auto t0 = std::chrono::steady_clock::now();
    aar_smooth_relative_report r;
    smooth_report_begin(pb, r);
    r.num_pairs = (int32_t)Q;
    if (Q > 0) {
        const int direct_lag = c.cv ? 3 : 1;   // the lags the selected inverse (and the lag-three blocks) hold
        for (size_t i = 0; i < Q; i++) {
            const int lag = std::abs(frame_a[i] - frame_b[i]);
            if (lag <= direct_lag) r.num_direct++; else r.num_chained++;
            r.max_lag = std::max(r.max_lag, lag);
        }
        const bool chained = r.num_chained > 0;
        if ((rc = c.begin(x_full))) return rc;
        // one allocation: cross [Q][36] | rel [Q][6] | rcov [Q][36] | the selected inverse's area | l3 [F-3][36] (constant velocity) | the gains
        // [K][144] or [F][36] | the pairs [2][Q] and two pivot flags: the lag-three blocks', the gains'
        const size_t n_sel = c.selinv_doubles(), n3 = c.cv ? 36 * (size_t)std::max(F - 3, 0) : 0;
        const size_t n_dbl = 78 * Q + n_sel + n3 + (c.cv ? 144 * (size_t)smooth_cv_nodes(F) : 36 * (size_t)F);
        DevMem out;
        if ((rc = out.alloc(pb, n_dbl, 2 * Q + 2))) return rc;
        double *d_cross = out.p, *d_rel = d_cross + 36 * Q, *d_rcov = d_rel + 6 * Q, *d_area = d_rcov + 36 * Q, *d_l3 = d_area + n_sel, *d_gain = d_l3 + n3;
        int32_t *d_fa = reinterpret_cast<int32_t *>(out.p + n_dbl), *d_fb = d_fa + Q, *d_flag = d_fb + Q;
        if ((rc = copy_h2d(pb, d_fa, frame_a, Q * sizeof(int32_t)))) return rc;
        if ((rc = copy_h2d(pb, d_fb, frame_b, Q * sizeof(int32_t)))) return rc;
        const SmoothSel sel = c.selinv(0, d_area);
        r.launches = sel.launches;
        if (c.cv) {
            r.launches += launch_smooth_cv_lag3(F, d_area, d_l3, d_flag, pb->stream);
            r.launches += launch_smooth_cv_relative(F, c.z(0), d_area, sel.fc, sel.lc, sel.l2, d_l3, d_gain, chained, (int64_t)Q, d_fa, d_fb, d_cross,
                                                    d_rel, d_rcov, d_flag + 1, pb->stream);
        } else {
            r.launches += launch_smooth_relative(F, c.z(0), sel.fc, sel.lc, d_gain, chained, (int64_t)Q, d_fa, d_fb, d_cross, d_rel, d_rcov, d_flag + 1,
                                                 pb->stream);
        }
        pb->launches += r.launches;
        double res[8];
        int32_t qflag[2] = {0, 0};
        if ((rc = c.read_pivot(who, "smoothing relative kernels", res))) return rc;
        if ((rc = copy_d2h(pb, qflag, d_flag, sizeof qflag))) return rc;
        if (qflag[0]) return set_error(AAR_ERR_NUMERIC, "%s: non-positive pivot in a supernode block of the lag-three blocks", who);
        if (qflag[1]) return set_error(AAR_ERR_NUMERIC, "%s: non-positive pivot in a covariance block that the chain inverts", who);
        r.data_cost = res[0]; r.prior_cost = res[1];
        if (cross_cov && (rc = copy_d2h(pb, cross_cov, d_cross, 36 * Q * sizeof(double)))) return rc;
        if (rel && (rc = copy_d2h(pb, rel, d_rel, 6 * Q * sizeof(double)))) return rc;
        if (rel_cov && (rc = copy_d2h(pb, rel_cov, d_rcov, 36 * Q * sizeof(double)))) return rc;
        if ((rc = check_async("smoothing relative kernels"))) return rc;
        HIP_TRY(hipStreamSynchronize(pb->stream));
    }
    smooth_report_end(r, report, t0);
    return AAR_OK;
}

// ------------------------------------------------------------------------------------------------
// Predicted corners with covariance, detection leverages (predict_kernels.hip)
// ------------------------------------------------------------------------------------------------
namespace {
struct PredictCall {
    void *base = nullptr;
    ~PredictCall() { if (base) (void)hipFree(base); }
};

int predict_refuse(const aar_problem *pb, const char *who) {
    if (pb->comm) return set_error(AAR_ERR_UNSUPPORTED, "%s: dense outputs are single-GPU only (as aar_eval_normal_equations)", who);
    if (pb->L.oi)
        return set_error(AAR_ERR_UNSUPPORTED, "%s: the problem optimises the camera intrinsics; its corners also depend on (fx, cx, fy, cy), whose "
                                              "columns the corner covariance does not carry yet (that is the next step)", who);
    return AAR_OK;
}

// The row mask without the covariance chain: what the chain reads off the diagonal of S -- an entity is determined when an observation,
// a pose prior or a pair prior touches it -- from the host's copies of the index structure
int predict_host_mask(aar_problem *pb, std::vector<int32_t> &mask) {
    const DeviceProblem &P = pb->P;
    const PoseLayout &L = pb->L;
    std::vector<char> touched((size_t)std::max(P.A, 1), 0);
    for (int32_t a : pb->h_fslot_ent) touched[a] = 1;
    for (const aar_pose_prior &p : pb->priors) touched[p.kind == AAR_PRIOR_CAMERA ? p.index : L.C + p.index] = 1;
    if (P.n_pair > 0) {
        std::vector<int32_t> ends(4 * (size_t)P.n_pair);
        if (int rc = copy_d2h(pb, ends.data(), P.pair_ends, ends.size() * sizeof(int32_t))) return rc;
        for (int p = 0; p < P.n_pair; p++) touched[ends[4 * (size_t)p]] = touched[ends[4 * (size_t)p + 1]] = 1;
    }
    mask.assign(P.n_pad, PREDICT_CONST);
    for (int a = 0; a < L.C + L.M; a++) {
        const bool zcol = a < L.C ? (L.oc && L.cam_slot(a) >= 0) : (L.om && L.mk_slot(a - L.C) >= 0);
        const int m = (!zcol || pb->h_ent_fixed[a]) ? PREDICT_CONST : (touched[a] ? PREDICT_LIVE : PREDICT_UNSEEN);
        for (int i = 0; i < 6; i++) mask[6 * (size_t)a + i] = m;
    }
    return AAR_OK;
}

// mode as launch_predict_corners: 0 = uv | cov | status, 1 = uv | status without the chain, 2 = the problem's own detections
int predict_run(aar_problem *pb, const double *x_full, int mode, int64_t n, const int32_t *q_cam, const int32_t *q_marker, const int32_t *q_frame,
                double *uv, double *cov, uint8_t *status, double *lev, double *row_lev, aar_predict_report *report) {
    const auto t0 = std::chrono::steady_clock::now();
    DeviceProblem &P = pb->P;
    const PoseLayout &L = pb->L;
    const int cur = pb->cur;
    const int64_t launches0 = pb->launches;
    aar_predict_report r;
    memset(&r, 0, sizeof r);
    r.num_residuals = 8 * pb->N_global;
    r.num_vars = L.z_len();
    r.sum_sq = r.sigma2 = NAN;
    std::vector<double> h_uv, h_cov, h_lev, h_row;
    std::vector<uint8_t> h_st;
    if (n > 0) {
        HIP_TRY(hipSetDevice(pb->device));
        int rc;
        CovChain ch;
        std::vector<int32_t> host_mask;
        if (mode != 1) {
            if ((rc = cov_chain(pb, x_full, true, false, ch))) return rc;
            r.sum_sq = ch.sum_sq;
            r.sigma2 = r.num_residuals > r.num_vars ? ch.sum_sq / (double)(r.num_residuals - r.num_vars) : NAN;
        } else {
            if ((rc = upload_z(pb, x_full, cur))) return rc;
            // whatever the LM state was, it is gone: z[cur] and its entity rows now hold x_full
            pb->lm_ready = false;
            pb->blocks_valid = false;
            pb->vinv_mu = pb->schur_mu = -1;
            pb->s_reduced = pb->trial_reduced = false;
            pb->spec_chol_blk = -1;
            if (pb->panels_blk == cur) pb->panels_blk = -1;
            if ((rc = predict_host_mask(pb, host_mask))) return rc;
        }
        const std::vector<int32_t> &mask = mode != 1 ? ch.mask : host_mask;
        for (int32_t m : mask) r.num_live_vars += m == PREDICT_LIVE;
        if (L.of)
            for (int f = 0; f < P.F; f++) r.num_live_vars += pb->h_fslot_start[f + 1] > pb->h_fslot_start[f] ? 6 : 0;
        const bool frames_opt = L.of && P.F > 0;
        // one allocation: gains | uv | cov | leverage | its rows, then the queries and the mask, then the status bytes
        const size_t N = (size_t)n, n_gain = (mode != 1 && frames_opt) ? 36 * (size_t)std::max(P.total_slots, 1) : 0, n_uv = mode != 2 ? 8 * N : 0,
                     n_cov = mode == 0 ? 64 * N : 0, n_lev = mode == 2 ? N : 0, n_row = mode == 2 ? 8 * N : 0;
        const size_t n_dbl = n_gain + n_uv + n_cov + n_lev + n_row, n_int = (mode != 2 ? 3 * N : 0) + (mode == 1 ? (size_t)P.n_pad : 0);
        const size_t bytes = n_dbl * sizeof(double) + n_int * sizeof(int32_t) + N;
        PredictCall out;
        HIP_TRY(hipMalloc(&out.base, bytes));
        HIP_TRY(hipMemsetAsync(out.base, 0, bytes, pb->stream));
        double *d_gain = static_cast<double *>(out.base), *d_uv = d_gain + n_gain, *d_cov = d_uv + n_uv, *d_lev = d_cov + n_cov, *d_row = d_lev + n_lev;
        int32_t *d_qc = reinterpret_cast<int32_t *>(d_row + n_row), *d_qm = d_qc + (mode != 2 ? N : 0), *d_qf = d_qm + (mode != 2 ? N : 0),
                *d_mask = d_qf + (mode != 2 ? N : 0);
        uint8_t *d_st = reinterpret_cast<uint8_t *>(reinterpret_cast<int32_t *>(d_row + n_row) + n_int);
        if (mode != 2 && ((rc = copy_h2d(pb, d_qc, q_cam, N * sizeof(int32_t))) || (rc = copy_h2d(pb, d_qm, q_marker, N * sizeof(int32_t))) ||
                          (rc = copy_h2d(pb, d_qf, q_frame, N * sizeof(int32_t)))))
            return rc;
        if (mode == 1 && (rc = copy_h2d(pb, d_mask, host_mask.data(), (size_t)P.n_pad * sizeof(int32_t)))) return rc;
        launch_unpack(P, cur, pb->stream);
        pb->launches += 1;
        const KTable kt = k_table(P, cur);
        PredictArgs a;
        memset(&a, 0, sizeof a);
        a.ent = P.ent[cur]; a.K = kt.base; a.kstride = kt.stride; a.C = P.C; a.A = P.A; a.h = P.half_size; a.n = n;
        a.q_cam = d_qc; a.q_marker = d_qm; a.q_frame = d_qf; a.obs = P.a_idx;
        a.fslot_start = P.fslot_start; a.fslot_ent = P.fslot_ent; a.rowmask = mode == 1 ? d_mask : ch.rowmask;
        a.frames_opt = frames_opt ? 1 : 0; a.n_pad = P.n_pad;
        a.gain = d_gain; a.Sinv = ch.Sinv; a.frame_cov = ch.frame_blocks;
        a.uv = d_uv; a.cov = d_cov; a.status = d_st; a.lev = d_lev; a.row_lev = (mode == 2 && row_lev) ? d_row : nullptr;
        if (mode != 1 && frames_opt) {
            launch_predict_gains(P, cur, ch.rowmask, d_gain, pb->stream);
            pb->launches += 1;
        }
        launch_predict_corners(a, mode, pb->stream);
        pb->launches += 1;
        if ((rc = check_async("predict kernels"))) return rc;
        HIP_TRY(hipStreamSynchronize(pb->stream));
        h_st.resize(N);
        if ((rc = copy_d2h(pb, h_st.data(), d_st, N))) return rc;
        if (mode != 2) { h_uv.resize(8 * N); if ((rc = copy_d2h(pb, h_uv.data(), d_uv, h_uv.size() * sizeof(double)))) return rc; }
        if (mode == 0) { h_cov.resize(64 * N); if ((rc = copy_d2h(pb, h_cov.data(), d_cov, h_cov.size() * sizeof(double)))) return rc; }
        if (mode == 2) { h_lev.resize(N); if ((rc = copy_d2h(pb, h_lev.data(), d_lev, N * sizeof(double)))) return rc; }
        if (mode == 2 && row_lev) { h_row.resize(8 * N); if ((rc = copy_d2h(pb, h_row.data(), d_row, h_row.size() * sizeof(double)))) return rc; }
        if ((rc = check_async("predict kernels"))) return rc;
        HIP_TRY(hipStreamSynchronize(pb->stream));
        // everything succeeded: only now the caller's arrays are written
        for (size_t i = 0; i < N; i++) {
            r.behind += (h_st[i] & AAR_PREDICT_BEHIND) ? 1 : 0;
            r.undefined += (h_st[i] & AAR_PREDICT_UNDEFINED) ? 1 : 0;
            double t = NAN;
            if (mode == 2) t = h_lev[i];
            if (mode == 0) {
                const double *c = &h_cov[64 * i];
                t = ((c[0] + c[9]) + (c[18] + c[27])) + ((c[36] + c[45]) + (c[54] + c[63]));   // (the kernel's order of the trace)
            }
            if (std::isfinite(t)) r.leverage_sum += t;
        }
        if (uv) memcpy(uv, h_uv.data(), h_uv.size() * sizeof(double));
        if (cov) memcpy(cov, h_cov.data(), h_cov.size() * sizeof(double));
        if (status) memcpy(status, h_st.data(), N);
        if (lev) memcpy(lev, h_lev.data(), N * sizeof(double));
        if (row_lev) memcpy(row_lev, h_row.data(), h_row.size() * sizeof(double));
    }
    r.launches = (int32_t)(pb->launches - launches0);
    r.seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    if (report) {
        r.struct_size = report->struct_size;
        memcpy(report, &r, std::min<size_t>(report->struct_size, sizeof r));
    }
    return AAR_OK;
}

// Leave-one-out residuals of the problem's own detections (mode 3) and the gate of candidate detections (mode 4): DESIGN.md section 37.
// One covariance chain, one gains launch, one query launch; the scalars the F statistic needs are on the host before that launch.
struct LooOut {
    double *w = nullptr, *q = nullptr, *F = nullptr, *cook = nullptr, *lev = nullptr, *margin = nullptr;
    uint8_t *status = nullptr, *keep = nullptr;
};

int loo_run(aar_problem *pb, const double *x_full, int mode, int64_t n, const int32_t *q_cam, const int32_t *q_marker, const int32_t *q_frame,
            const float *uv_obs, double f_max, const LooOut &o, aar_predict_report &r, aar_loo_report *lr) {
    const auto t0 = std::chrono::steady_clock::now();
    DeviceProblem &P = pb->P;
    const PoseLayout &L = pb->L;
    const int cur = pb->cur;
    const int64_t launches0 = pb->launches;
    memset(&r, 0, sizeof r);
    r.num_residuals = 8 * pb->N_global;
    r.num_vars = L.z_len();
    r.sum_sq = r.sigma2 = NAN;
    const int64_t dof = r.num_residuals - r.num_vars;
    if (lr) {
        lr->dof = dof; lr->undetermined = lr->rejected = 0; lr->f_max = f_max > 0.0 ? f_max : INFINITY;
        lr->max_f = NAN; lr->argmax_f = -1;
    }
    if (n > 0) {
        HIP_TRY(hipSetDevice(pb->device));
        int rc;
        CovChain ch;
        if ((rc = cov_chain(pb, x_full, true, false, ch))) return rc;
        r.sum_sq = ch.sum_sq;
        r.sigma2 = dof > 0 ? ch.sum_sq / (double)dof : NAN;
        for (int32_t m : ch.mask) r.num_live_vars += m == PREDICT_LIVE;
        if (L.of)
            for (int f = 0; f < P.F; f++) r.num_live_vars += pb->h_fslot_start[f + 1] > pb->h_fslot_start[f] ? 6 : 0;
        const bool frames_opt = L.of && P.F > 0;
        // one allocation: gains | w | q | k | margin | F | cook | leverage, then the queries and the caller's corners, then status | keep
        const size_t N = (size_t)n, n_gain = frames_opt ? 36 * (size_t)std::max(P.total_slots, 1) : 0, n_m3 = mode == 3 ? N : 0;
        const size_t n_dbl = n_gain + 8 * N + 3 * N + 3 * n_m3, n_int = mode == 4 ? 3 * N : 0, n_flt = mode == 4 ? 8 * N : 0;
        const size_t bytes = n_dbl * sizeof(double) + n_int * sizeof(int32_t) + n_flt * sizeof(float) + 2 * N;
        PredictCall out;
        HIP_TRY(hipMalloc(&out.base, bytes));
        HIP_TRY(hipMemsetAsync(out.base, 0, bytes, pb->stream));
        double *d_gain = static_cast<double *>(out.base), *d_w = d_gain + n_gain, *d_q = d_w + 8 * N, *d_k = d_q + N, *d_mg = d_k + N, *d_F = d_mg + N,
               *d_ck = d_F + n_m3, *d_lev = d_ck + n_m3, *d_end = d_lev + n_m3;   // (k is mode 3's: its slot stays zero in mode 4)
        int32_t *d_qc = reinterpret_cast<int32_t *>(d_end), *d_qm = d_qc + (mode == 4 ? N : 0), *d_qf = d_qm + (mode == 4 ? N : 0);
        float *d_obs = reinterpret_cast<float *>(d_qc + n_int);
        uint8_t *d_st = reinterpret_cast<uint8_t *>(d_obs + n_flt), *d_keep = d_st + N;
        if (mode == 4 && ((rc = copy_h2d(pb, d_qc, q_cam, N * sizeof(int32_t))) || (rc = copy_h2d(pb, d_qm, q_marker, N * sizeof(int32_t))) ||
                          (rc = copy_h2d(pb, d_qf, q_frame, N * sizeof(int32_t))) || (rc = copy_h2d(pb, d_obs, uv_obs, 8 * N * sizeof(float)))))
            return rc;
        launch_unpack(P, cur, pb->stream);
        pb->launches += 1;
        const KTable kt = k_table(P, cur);
        PredictArgs a;
        memset(&a, 0, sizeof a);
        a.ent = P.ent[cur]; a.K = kt.base; a.kstride = kt.stride; a.C = P.C; a.A = P.A; a.h = P.half_size; a.n = n;
        a.q_cam = d_qc; a.q_marker = d_qm; a.q_frame = d_qf; a.obs = P.a_idx;
        a.fslot_start = P.fslot_start; a.fslot_ent = P.fslot_ent; a.rowmask = ch.rowmask;
        a.frames_opt = frames_opt ? 1 : 0; a.n_pad = P.n_pad;
        a.gain = d_gain; a.Sinv = ch.Sinv; a.frame_cov = ch.frame_blocks;
        a.status = d_st; a.lev = d_lev;
        a.obs_uv = mode == 3 ? P.a_uv : d_obs;
        a.loo_w = d_w; a.loo_q = d_q; a.loo_k = d_k; a.loo_margin = d_mg; a.loo_F = d_F; a.loo_cook = d_ck; a.loo_keep = d_keep;
        a.sum_sq = r.sum_sq; a.cook_den = (double)r.num_live_vars * r.sigma2; a.f_max = f_max > 0.0 ? f_max : 0.0; a.dof = dof;
        if (frames_opt) {
            launch_predict_gains(P, cur, ch.rowmask, d_gain, pb->stream);
            pb->launches += 1;
        }
        launch_predict_corners(a, mode, pb->stream);
        pb->launches += 1;
        if ((rc = check_async("leave-one-out kernels"))) return rc;
        HIP_TRY(hipStreamSynchronize(pb->stream));
        // to the host: what the report needs (status | keep, and for mode 3 F and the leverage) and what the caller asked for, nothing else,
        // into staging that nobody has touched before (no fill pass); the caller's arrays are written below, after every copy succeeded
        std::unique_ptr<double[]> h_d(new double[(size_t)(d_end - d_w)]);
        std::vector<uint8_t> h_b(2 * N);
        double *h_w = h_d.get(), *h_q = h_w + 8 * N, *h_mg = h_q + 2 * N, *h_F = h_mg + N, *h_ck = h_F + n_m3, *h_lev = h_ck + n_m3;
        if ((rc = copy_d2h(pb, h_b.data(), d_st, 2 * N))) return rc;
        if (o.w && (rc = copy_d2h(pb, h_w, d_w, 8 * N * sizeof(double)))) return rc;
        if (o.q && (rc = copy_d2h(pb, h_q, d_q, N * sizeof(double)))) return rc;
        if (o.margin && (rc = copy_d2h(pb, h_mg, d_mg, N * sizeof(double)))) return rc;
        if (mode == 3 && ((rc = copy_d2h(pb, h_F, d_F, N * sizeof(double))) || (rc = copy_d2h(pb, h_lev, d_lev, N * sizeof(double))))) return rc;
        if (mode == 3 && o.cook && (rc = copy_d2h(pb, h_ck, d_ck, N * sizeof(double)))) return rc;
        if ((rc = check_async("leave-one-out kernels"))) return rc;
        HIP_TRY(hipStreamSynchronize(pb->stream));
        // everything succeeded: only now the caller's arrays are written
        for (size_t i = 0; i < N; i++) {
            r.behind += (h_b[i] & AAR_PREDICT_BEHIND) ? 1 : 0;
            r.undefined += (h_b[i] & AAR_PREDICT_UNDEFINED) ? 1 : 0;
            if (mode == 3 && std::isfinite(h_lev[i])) r.leverage_sum += h_lev[i];
            if (lr && mode == 3) {
                lr->undetermined += (h_b[i] & AAR_PREDICT_UNDETERMINED) ? 1 : 0;
                lr->rejected += h_b[N + i] ? 0 : 1;
                if (h_F[i] > lr->max_f || (lr->argmax_f < 0 && !std::isnan(h_F[i]))) { lr->max_f = h_F[i]; lr->argmax_f = (int64_t)i; }
            }
        }
        if (o.w) memcpy(o.w, h_w, 8 * N * sizeof(double));
        if (o.q) memcpy(o.q, h_q, N * sizeof(double));
        if (o.margin) memcpy(o.margin, h_mg, N * sizeof(double));
        if (o.status) memcpy(o.status, h_b.data(), N);
        if (mode == 3) {
            if (o.F) memcpy(o.F, h_F, N * sizeof(double));
            if (o.cook) memcpy(o.cook, h_ck, N * sizeof(double));
            if (o.lev) memcpy(o.lev, h_lev, N * sizeof(double));
            if (o.keep) memcpy(o.keep, h_b.data() + N, N);
        }
    }
    r.launches = (int32_t)(pb->launches - launches0);
    r.seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    return AAR_OK;
}
}  // namespace

int aar_problem_predict_corners(aar_problem *pb, const double *x_full, int64_t n_query, const int32_t *q_cam, const int32_t *q_marker,
                                const int32_t *q_frame, double *uv, double *cov, uint8_t *status, aar_predict_report *report) {
    if (!pb) {   // no problem exists without a device: say which of the two it is
        if (int rc = ensure_device(0)) return rc;
        return set_error(AAR_ERR_INVALID, "aar_problem_predict_corners: null problem");
    }
    if (!x_full || (n_query > 0 && !uv)) return set_error(AAR_ERR_INVALID, "aar_problem_predict_corners: null argument");
    if (report && report->struct_size < sizeof(uint32_t)) return set_error(AAR_ERR_INVALID, "aar_problem_predict_corners: report->struct_size not set");
    int rc = predict_refuse(pb, "aar_problem_predict_corners");
    if (rc) return rc;
    aar_problem_desc d;
    memset(&d, 0, sizeof d);
    d.num_cams = pb->L.C; d.num_markers = pb->L.M; d.num_frames = pb->L.F;
    if ((rc = aar_predict_query_validate(&d, n_query, q_cam, q_marker, q_frame))) return rc;
    return predict_run(pb, x_full, cov ? 0 : 1, n_query, q_cam, q_marker, q_frame, uv, cov, status, nullptr, nullptr, report);
}

int aar_problem_detection_leverage(aar_problem *pb, const double *x_full, double *leverage, double *row_leverage, aar_predict_report *report) {
    if (!pb) {
        if (int rc = ensure_device(0)) return rc;
        return set_error(AAR_ERR_INVALID, "aar_problem_detection_leverage: null problem");
    }
    if (!x_full || (pb->P.N > 0 && !leverage)) return set_error(AAR_ERR_INVALID, "aar_problem_detection_leverage: null argument");
    if (report && report->struct_size < sizeof(uint32_t)) return set_error(AAR_ERR_INVALID, "aar_problem_detection_leverage: report->struct_size not set");
    int rc = predict_refuse(pb, "aar_problem_detection_leverage");
    if (rc) return rc;
    return predict_run(pb, x_full, 2, pb->P.N, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, leverage, row_leverage, report);
}

int aar_problem_detection_loo(aar_problem *pb, const double *x_full, const aar_loo_rule *rule, double *loo_resid, double *q, double *F, double *cook,
                              double *leverage, double *margin, uint8_t *status, uint8_t *keep, aar_loo_report *report) {
    if (!pb) {
        if (int rc = ensure_device(0)) return rc;
        return set_error(AAR_ERR_INVALID, "aar_problem_detection_loo: null problem");
    }
    if (!x_full) return set_error(AAR_ERR_INVALID, "aar_problem_detection_loo: null argument");
    if (report && report->struct_size < sizeof(uint32_t)) return set_error(AAR_ERR_INVALID, "aar_problem_detection_loo: report->struct_size not set");
    if (rule) {
        if (rule->struct_size < offsetof(aar_loo_rule, f_max) + sizeof(double))
            return set_error(AAR_ERR_INVALID, "aar_problem_detection_loo: rule->struct_size %u does not reach f_max", (unsigned)rule->struct_size);
        if (!(rule->f_max > 0.0) || !std::isfinite(rule->f_max))
            return set_error(AAR_ERR_INVALID, "aar_problem_detection_loo: rule->f_max = %g must be positive and finite", rule->f_max);
    }
    int rc = predict_refuse(pb, "aar_problem_detection_loo");
    if (rc) return rc;
    if (pb->with_huber)
        return set_error(AAR_ERR_UNSUPPORTED, "aar_problem_detection_loo: the problem was created with_huber; the Huber weights break the Gaussian "
                                              "data model the statistic rests on");
    aar_loo_report r;
    memset(&r, 0, sizeof r);
    LooOut o;
    o.w = loo_resid; o.q = q; o.F = F; o.cook = cook; o.lev = leverage; o.margin = margin; o.status = status; o.keep = keep;
    if ((rc = loo_run(pb, x_full, 3, pb->P.N, nullptr, nullptr, nullptr, nullptr, rule ? rule->f_max : 0.0, o, r.predict, &r))) return rc;
    r.predict.struct_size = sizeof(aar_predict_report);
    if (report) {
        r.struct_size = report->struct_size;
        memcpy(report, &r, std::min<size_t>(report->struct_size, sizeof r));
    }
    return AAR_OK;
}

int aar_problem_gate_detections(aar_problem *pb, const double *x_full, int64_t n_query, const int32_t *q_cam, const int32_t *q_marker,
                                const int32_t *q_frame, const float *uv_obs, double *innovation, double *m2, uint8_t *status,
                                aar_predict_report *report) {
    if (!pb) {
        if (int rc = ensure_device(0)) return rc;
        return set_error(AAR_ERR_INVALID, "aar_problem_gate_detections: null problem");
    }
    if (!x_full || (n_query > 0 && !uv_obs)) return set_error(AAR_ERR_INVALID, "aar_problem_gate_detections: null argument");
    if (report && report->struct_size < sizeof(uint32_t)) return set_error(AAR_ERR_INVALID, "aar_problem_gate_detections: report->struct_size not set");
    int rc = predict_refuse(pb, "aar_problem_gate_detections");
    if (rc) return rc;
    aar_problem_desc d;
    memset(&d, 0, sizeof d);
    d.num_cams = pb->L.C; d.num_markers = pb->L.M; d.num_frames = pb->L.F;
    if ((rc = aar_predict_query_validate(&d, n_query, q_cam, q_marker, q_frame))) return rc;
    aar_predict_report r;
    LooOut o;
    o.w = innovation; o.q = m2; o.status = status;
    if ((rc = loo_run(pb, x_full, 4, n_query, q_cam, q_marker, q_frame, uv_obs, 0.0, o, r, nullptr))) return rc;
    if (report) {
        r.struct_size = report->struct_size;
        memcpy(report, &r, std::min<size_t>(report->struct_size, sizeof r));
    }
    return AAR_OK;
}

// ------------------------------------------------------------------------------------------------
// The same per-detection layer on a smoothed track (smooth_predict_kernels.hip)
// ------------------------------------------------------------------------------------------------
namespace {

// the launch of k_smooth_corners between two events when the problem's kernel profiling is on (aar_set_kernel_profiling): its own time for
// the reports' kernel_seconds, read after the call's last synchronisation; 0 otherwise
struct SmoothCornersTimer {
    hipEvent_t e0 = nullptr, e1 = nullptr;
    ~SmoothCornersTimer() { if (e0) (void)hipEventDestroy(e0); if (e1) (void)hipEventDestroy(e1); }
    void launch(const aar_problem *pb, const SmoothCornersArgs &a, int mode) {
        const bool on = pb->profiling && hipEventCreate(&e0) == hipSuccess && hipEventCreate(&e1) == hipSuccess;
        if (on) (void)hipEventRecord(e0, pb->stream);
        launch_smooth_corners(a, mode, pb->stream);
        if (on) (void)hipEventRecord(e1, pb->stream);
        else if (e0) { (void)hipEventDestroy(e0); e0 = nullptr; }
    }
    double seconds() const {
        float ms = 0.f;
        return e0 && e1 && hipEventElapsedTime(&ms, e0, e1) == hipSuccess ? 1e-3 * (double)ms : 0.0;
    }
};

// what the kernel reads of the problem itself
SmoothCornersArgs smooth_corners_args(const aar_problem *pb, int64_t n) {
    const DeviceProblem &P = pb->P;
    const KTable kt = k_table(P, pb->cur);
    SmoothCornersArgs a;
    memset(&a, 0, sizeof a);
    a.ent = P.ent[pb->cur]; a.K = kt.base; a.kstride = kt.stride; a.C = P.C; a.h = P.half_size; a.n = n;
    a.obs = P.a_idx;
    return a;
}

// aar_track_smooth_detection_leverage (mode 2) and aar_track_smooth_detection_loo (mode 3) after their checks: the chain of
// aar_track_smooth_covariance2, whose diagonal blocks stay on the device, and one launch over the problem's detections behind it.  r: the
// report's head (costs, launches); hb: status | keep of every detection, hF, hlev: what the report's counts need (mode 3)
extern "C++" template <class R>
int smooth_detections(SmoothRun &c, const char *who, const double *x_full, int mode, double f_max, const LooOut &o, double *row_lev, R &r,
                      std::vector<uint8_t> &h_b, std::vector<double> &h_F, std::vector<double> &h_lev) {
    aar_problem *pb = c.pb;
    DeviceProblem &P = pb->P;
    const int F = P.F;
    const size_t N = (size_t)P.N;
    int rc = c.begin(x_full);
    if (rc) return rc;
    if (F == 0) { HIP_TRY(hipStreamSynchronize(pb->stream)); return AAR_OK; }
    // one allocation: the selected inverse's area | w [N][8] (mode 3) or the rows [N][8] (mode 2) | q | margin | F | cook | leverage, then
    // status | keep
    const size_t n_sel = c.selinv_doubles(), n_m3 = mode == 3 ? N : 0;
    const size_t n_dbl = n_sel + 8 * N + 2 * n_m3 + 2 * n_m3 + N, n_bytes = 2 * N;
    DevMem out;
    if ((rc = out.alloc(pb, n_dbl, (n_bytes + 3) / 4))) return rc;
    double *d_w = out.p + n_sel, *d_q = d_w + 8 * N, *d_mg = d_q + n_m3, *d_F = d_mg + n_m3, *d_ck = d_F + n_m3, *d_lev = d_ck + n_m3;
    uint8_t *d_st = reinterpret_cast<uint8_t *>(out.p + n_dbl), *d_keep = d_st + N;
    const SmoothSel sel = c.selinv(0, out.p);
    r.launches = sel.launches;
    SmoothCornersTimer timer;
    if (N > 0) {
        SmoothCornersArgs a = smooth_corners_args(pb, (int64_t)N);
        a.pose = c.z(0); a.block = sel.fc;
        a.status = d_st; a.lev = d_lev; a.row_lev = (mode == 2 && row_lev) ? d_w : nullptr;
        a.obs_uv = P.a_uv;
        a.loo_w = d_w; a.loo_q = d_q; a.loo_margin = d_mg; a.loo_F = d_F; a.loo_cook = d_ck; a.loo_keep = d_keep;
        a.res = c.res(); a.f_max = f_max > 0.0 ? f_max : 0.0; a.num_vars = (double)r.num_vars; a.dof = r.num_residuals - r.num_vars;
        timer.launch(pb, a, mode);
        r.launches += 1;
    }
    pb->launches += r.launches;
    double res[8];
    if ((rc = c.read_pivot(who, "smoothing covariance kernels", res))) return rc;
    r.data_cost = res[0]; r.prior_cost = res[1];
    if (N == 0) return AAR_OK;
    // to the host, into staging: what the report needs and what the caller asked for; the caller's arrays are written after every copy succeeded
    std::unique_ptr<double[]> h_w, h_q, h_mg, h_ck;
    h_b.resize(2 * N);
    h_lev.resize(N);
    if ((rc = copy_d2h(pb, h_b.data(), d_st, 2 * N))) return rc;
    if ((rc = copy_d2h(pb, h_lev.data(), d_lev, N * sizeof(double)))) return rc;
    if (mode == 2 ? row_lev != nullptr : o.w != nullptr) {
        h_w.reset(new double[8 * N]);
        if ((rc = copy_d2h(pb, h_w.get(), d_w, 8 * N * sizeof(double)))) return rc;
    }
    if (mode == 3) {
        h_F.resize(N);
        if ((rc = copy_d2h(pb, h_F.data(), d_F, N * sizeof(double)))) return rc;
        if (o.q) { h_q.reset(new double[N]); if ((rc = copy_d2h(pb, h_q.get(), d_q, N * sizeof(double)))) return rc; }
        if (o.margin) { h_mg.reset(new double[N]); if ((rc = copy_d2h(pb, h_mg.get(), d_mg, N * sizeof(double)))) return rc; }
        if (o.cook) { h_ck.reset(new double[N]); if ((rc = copy_d2h(pb, h_ck.get(), d_ck, N * sizeof(double)))) return rc; }
    }
    if ((rc = check_async("smoothing detection kernels"))) return rc;
    HIP_TRY(hipStreamSynchronize(pb->stream));
    r.kernel_seconds = timer.seconds();
    // everything succeeded: only now the caller's arrays are written
    if (o.lev) memcpy(o.lev, h_lev.data(), N * sizeof(double));
    if (mode == 2 && row_lev) memcpy(row_lev, h_w.get(), 8 * N * sizeof(double));
    if (mode == 3) {
        if (o.w) memcpy(o.w, h_w.get(), 8 * N * sizeof(double));
        if (o.q) memcpy(o.q, h_q.get(), N * sizeof(double));
        if (o.margin) memcpy(o.margin, h_mg.get(), N * sizeof(double));
        if (o.cook) memcpy(o.cook, h_ck.get(), N * sizeof(double));
        if (o.F) memcpy(o.F, h_F.data(), N * sizeof(double));
        if (o.status) memcpy(o.status, h_b.data(), N);
        if (o.keep) memcpy(o.keep, h_b.data() + N, N);
    }
    return AAR_OK;
}

// aar_track_smooth_predict_corners (mode 0, or 1 without cov) and aar_track_smooth_gate_detections (mode 4) after smooth_entry: the checks,
// the query chain of aar_track_smooth_query2, whose poses and blocks stay on the device, and one launch over the queries behind it
int smooth_time_queries(SmoothRun &c, const char *who, const double *x_full, const aar_smooth_params *sp_in, int mode, int64_t n_query,
                        const int32_t *q_cam, const int32_t *q_marker, const double *q_time, const float *uv_obs, double *uv, double *cov,
                        double *m2, uint8_t *status, int32_t *segment, aar_smooth_predict_report *report) {
    aar_problem *pb = c.pb;
    int rc = aar_smooth_query_validate(pb->L.F, sp_in, n_query, q_time);
    if (rc) return rc;
    if (n_query > 0 && (!q_cam || !q_marker)) return set_error(AAR_ERR_INVALID, "%s: null query array with n_query = %lld", who, (long long)n_query);
    for (int64_t i = 0; i < n_query; i++) {
        if (q_cam[i] < 0 || q_cam[i] >= pb->L.C)
            return set_error(AAR_ERR_INVALID, "%s: q_cam[%lld] = %d lies outside 0 .. num_cams - 1 = %d", who, (long long)i, (int)q_cam[i], pb->L.C - 1);
        if (q_marker[i] < 0 || q_marker[i] >= pb->L.M)
            return set_error(AAR_ERR_INVALID, "%s: q_marker[%lld] = %d lies outside 0 .. num_markers - 1 = %d", who, (long long)i, (int)q_marker[i],
                             pb->L.M - 1);
    }
    if (c.sp.rel_motion)
        return set_error(AAR_ERR_UNSUPPORTED, "%s: rel_motion is set; under an expected motion the pose of an inserted frame "
                                              "has no closed form (the split of dR does not commute)", who);
    const size_t Q = (size_t)n_query;
    const auto t0 = std::chrono::steady_clock::now();
    aar_smooth_predict_report r;
    smooth_report_begin(pb, r);
    r.num_queries = (int64_t)Q;
    if (Q > 0) {
        DeviceProblem &P = pb->P;
        aar_smooth_query_report counts;
        memset(&counts, 0, sizeof counts);
        std::vector<double> ft;
        smooth_query_times(c.sp, P.F, Q, q_time, ft, counts);
        r.num_inside = counts.num_inside; r.num_on_frame = counts.num_on_frame; r.num_outside = counts.num_outside;
        SmoothQueryDev d;
        if ((rc = smooth_query_device(c, x_full, Q, q_time, ft, mode != 1, d))) return rc;
        r.launches = d.launches;
        if (!d.blocks) {   // (no work area, and nobody has made the rows of the cameras and markers yet)
            launch_unpack(P, pb->cur, pb->stream);
            r.launches += 1;
        }
        // one allocation: uv [Q][8] (the gate: the innovation) | cov [Q][64] (mode 0) | m2, margin [Q] (mode 4), then the caller's corners
        // (mode 4), the queries' cameras and markers, the status bytes
        const size_t n_cov = mode == 0 ? 64 * Q : 0, n_m4 = mode == 4 ? Q : 0, n_dbl = 8 * Q + n_cov + 2 * n_m4;
        DevMem out;
        if ((rc = out.alloc(pb, n_dbl, 8 * n_m4 + 2 * Q + (Q + 3) / 4))) return rc;
        double *d_uv = out.p, *d_cov = d_uv + 8 * Q, *d_m2 = d_cov + n_cov, *d_mg = d_m2 + n_m4;
        float *d_obs = reinterpret_cast<float *>(out.p + n_dbl);
        int32_t *d_qc = reinterpret_cast<int32_t *>(d_obs + 8 * n_m4), *d_qm = d_qc + Q;
        uint8_t *d_st = reinterpret_cast<uint8_t *>(d_qm + Q);
        if ((rc = copy_h2d(pb, d_qc, q_cam, Q * sizeof(int32_t))) || (rc = copy_h2d(pb, d_qm, q_marker, Q * sizeof(int32_t)))) return rc;
        if (mode == 4 && (rc = copy_h2d(pb, d_obs, uv_obs, 8 * Q * sizeof(float)))) return rc;
        SmoothCornersArgs a = smooth_corners_args(pb, (int64_t)Q);
        a.q_cam = d_qc; a.q_marker = d_qm; a.pose = d.pose; a.block = d.cov;
        a.uv = d_uv; a.cov = d_cov; a.status = d_st;
        a.obs_uv = d_obs; a.loo_w = d_uv; a.loo_q = d_m2; a.loo_margin = d_mg;
        SmoothCornersTimer timer;
        timer.launch(pb, a, mode);
        r.launches += 1;
        pb->launches += r.launches;
        if (d.blocks) {
            double res[8];
            if ((rc = smooth_query_pivots(c, who, d, res))) return rc;
            r.data_cost = res[0]; r.prior_cost = res[1];
        }
        std::vector<uint8_t> h_st(Q);
        std::vector<int32_t> h_seg(Q);
        std::unique_ptr<double[]> h_uv(new double[8 * Q]), h_cov, h_m2;
        if ((rc = copy_d2h(pb, h_st.data(), d_st, Q))) return rc;
        if ((rc = copy_d2h(pb, h_seg.data(), d.seg, Q * sizeof(int32_t)))) return rc;
        if ((rc = copy_d2h(pb, h_uv.get(), d_uv, 8 * Q * sizeof(double)))) return rc;
        if (mode == 0) { h_cov.reset(new double[64 * Q]); if ((rc = copy_d2h(pb, h_cov.get(), d_cov, 64 * Q * sizeof(double)))) return rc; }
        if (mode == 4) { h_m2.reset(new double[Q]); if ((rc = copy_d2h(pb, h_m2.get(), d_m2, Q * sizeof(double)))) return rc; }
        if ((rc = check_async("smoothing detection kernels"))) return rc;
        HIP_TRY(hipStreamSynchronize(pb->stream));
        r.kernel_seconds = timer.seconds();
        // everything succeeded: only now the caller's arrays are written
        for (size_t i = 0; i < Q; i++) {
            r.behind += (h_st[i] & AAR_PREDICT_BEHIND) ? 1 : 0;
            if (mode == 0) {
                const double *cc = &h_cov[64 * i];
                const double t = ((cc[0] + cc[9]) + (cc[18] + cc[27])) + ((cc[36] + cc[45]) + (cc[54] + cc[63]));   // (the kernel's order of the trace)
                if (std::isfinite(t)) r.leverage_sum += t;
            }
        }
        if (uv) memcpy(uv, h_uv.get(), 8 * Q * sizeof(double));
        if (cov) memcpy(cov, h_cov.get(), 64 * Q * sizeof(double));
        if (m2) memcpy(m2, h_m2.get(), Q * sizeof(double));
        if (status) memcpy(status, h_st.data(), Q);
        if (segment) memcpy(segment, h_seg.data(), Q * sizeof(int32_t));
    }
    smooth_report_end(r, report, t0);
    return AAR_OK;
}

}  // namespace

int aar_track_smooth_detection_leverage(aar_problem *pb, const double *x_full, const aar_smooth_params *sp_in, double *leverage, double *row_leverage,
                                        aar_smooth_predict_report *report) {
    const char *who = "aar_track_smooth_detection_leverage";
    if (!pb || !x_full || (pb->P.N > 0 && !leverage)) return set_error(AAR_ERR_INVALID, "%s: null argument", who);
    if (report && report->struct_size < sizeof(uint32_t)) return set_error(AAR_ERR_INVALID, "%s: report->struct_size not set", who);
    SmoothRun c;
    int rc = smooth_entry(pb, sp_in, c, who);
    if (rc) return rc;
    const auto t0 = std::chrono::steady_clock::now();
    aar_smooth_predict_report r;
    smooth_report_begin(pb, r);
    r.num_queries = pb->P.N;
    LooOut o;
    o.lev = leverage;
    std::vector<uint8_t> h_b;
    std::vector<double> h_F, h_lev;
    if ((rc = smooth_detections(c, who, x_full, 2, 0.0, o, row_leverage, r, h_b, h_F, h_lev))) return rc;
    for (size_t i = 0; i < h_lev.size(); i++) {
        r.behind += (h_b[i] & AAR_PREDICT_BEHIND) ? 1 : 0;
        if (std::isfinite(h_lev[i])) r.leverage_sum += h_lev[i];
    }
    smooth_report_end(r, report, t0);
    return AAR_OK;
}

int aar_track_smooth_detection_loo(aar_problem *pb, const double *x_full, const aar_smooth_params *sp_in, const aar_loo_rule *rule, double *loo_resid,
                                   double *q, double *F, double *cook, double *leverage, double *margin, uint8_t *status, uint8_t *keep,
                                   aar_smooth_loo_report *report) {
    const char *who = "aar_track_smooth_detection_loo";
    if (!pb || !x_full) return set_error(AAR_ERR_INVALID, "%s: null argument", who);
    if (report && report->struct_size < sizeof(uint32_t)) return set_error(AAR_ERR_INVALID, "%s: report->struct_size not set", who);
    if (rule) {
        if (rule->struct_size < offsetof(aar_loo_rule, f_max) + sizeof(double))
            return set_error(AAR_ERR_INVALID, "%s: rule->struct_size %u does not reach f_max", who, (unsigned)rule->struct_size);
        if (!(rule->f_max > 0.0) || !std::isfinite(rule->f_max))
            return set_error(AAR_ERR_INVALID, "%s: rule->f_max = %g must be positive and finite", who, rule->f_max);
    }
    SmoothRun c;
    int rc = smooth_entry(pb, sp_in, c, who);
    if (rc) return rc;
    if (pb->with_huber)
        return set_error(AAR_ERR_UNSUPPORTED, "%s: the problem was created with_huber; the Huber weights break the Gaussian data model the "
                                              "statistic rests on", who);
    const auto t0 = std::chrono::steady_clock::now();
    aar_smooth_loo_report r;
    smooth_report_begin(pb, r);
    r.dof = r.num_residuals - r.num_vars;
    r.f_max = rule ? rule->f_max : INFINITY;
    r.max_f = NAN;
    r.argmax_f = -1;
    LooOut o;
    o.w = loo_resid; o.q = q; o.F = F; o.cook = cook; o.lev = leverage; o.margin = margin; o.status = status; o.keep = keep;
    std::vector<uint8_t> h_b;
    std::vector<double> h_F, h_lev;
    if ((rc = smooth_detections(c, who, x_full, 3, rule ? rule->f_max : 0.0, o, nullptr, r, h_b, h_F, h_lev))) return rc;
    const size_t N = h_lev.size();
    for (size_t i = 0; i < N; i++) {
        r.behind += (h_b[i] & AAR_PREDICT_BEHIND) ? 1 : 0;
        r.undetermined += (h_b[i] & AAR_PREDICT_UNDETERMINED) ? 1 : 0;
        r.rejected += h_b[N + i] ? 0 : 1;
        if (std::isfinite(h_lev[i])) r.leverage_sum += h_lev[i];
        if (h_F[i] > r.max_f || (r.argmax_f < 0 && !std::isnan(h_F[i]))) { r.max_f = h_F[i]; r.argmax_f = (int64_t)i; }
    }
    smooth_report_end(r, report, t0);
    return AAR_OK;
}

int aar_track_smooth_predict_corners(aar_problem *pb, const double *x_full, const aar_smooth_params *sp_in, int64_t n_query, const int32_t *q_cam,
                                     const int32_t *q_marker, const double *q_time, double *uv, double *cov, uint8_t *status, int32_t *segment,
                                     aar_smooth_predict_report *report) {
    const char *who = "aar_track_smooth_predict_corners";
    if (!pb || !x_full || (n_query > 0 && !uv)) return set_error(AAR_ERR_INVALID, "%s: null argument", who);
    if (report && report->struct_size < sizeof(uint32_t)) return set_error(AAR_ERR_INVALID, "%s: report->struct_size not set", who);
    SmoothRun c;
    int rc = smooth_entry(pb, sp_in, c, who);
    if (rc) return rc;
    return smooth_time_queries(c, who, x_full, sp_in, cov ? 0 : 1, n_query, q_cam, q_marker, q_time, nullptr, uv, cov, nullptr, status, segment, report);
}

int aar_track_smooth_gate_detections(aar_problem *pb, const double *x_full, const aar_smooth_params *sp_in, int64_t n_query, const int32_t *q_cam,
                                     const int32_t *q_marker, const double *q_time, const float *uv_obs, double *innovation, double *m2,
                                     uint8_t *status, int32_t *segment, aar_smooth_predict_report *report) {
    const char *who = "aar_track_smooth_gate_detections";
    if (!pb || !x_full || (n_query > 0 && !uv_obs)) return set_error(AAR_ERR_INVALID, "%s: null argument", who);
    if (report && report->struct_size < sizeof(uint32_t)) return set_error(AAR_ERR_INVALID, "%s: report->struct_size not set", who);
    SmoothRun c;
    int rc = smooth_entry(pb, sp_in, c, who);
    if (rc) return rc;
    return smooth_time_queries(c, who, x_full, sp_in, 4, n_query, q_cam, q_marker, q_time, uv_obs, innovation, nullptr, m2, status, segment, report);
}

int aar_set_kernel_profiling(aar_problem *pb, int on) {
    if (!pb) return set_error(AAR_ERR_INVALID, "aar_set_kernel_profiling: null argument");
    HIP_TRY(hipSetDevice(pb->device));
    HIP_TRY(hipStreamSynchronize(pb->stream));
    pb->ev_kid.clear();
    pb->ev_used = 0;
    pb->profiling = on != 0;
    if (on) {
        memset(pb->k_seconds, 0, sizeof pb->k_seconds);
        memset(pb->k_launches, 0, sizeof pb->k_launches);
        pb->P.hook.pre = prof_pre;
        pb->P.hook.post = prof_post;
        pb->P.hook.ctx = pb;
    } else {
        pb->P.hook = LaunchHook();
    }
    return AAR_OK;
}

int aar_get_kernel_times(aar_problem *pb, double seconds[AAR_NUM_KERNELS], int64_t launches[AAR_NUM_KERNELS]) {
    if (!pb || !seconds || !launches) return set_error(AAR_ERR_INVALID, "aar_get_kernel_times: null argument");
    static_assert(AAR_NUM_KERNELS == KID_COUNT, "kernel id table out of sync with include/aar.h");
    static_assert(ENT_STRIDE == ENT_STRIDE_H, "entity row stride");
    HIP_TRY(hipSetDevice(pb->device));
    HIP_TRY(hipStreamSynchronize(pb->stream));
    prof_harvest(pb);
    for (int i = 0; i < KID_COUNT; i++) { seconds[i] = pb->k_seconds[i]; launches[i] = pb->k_launches[i]; }
    return AAR_OK;
}

const char *aar_kernel_name(int kid) {
    static const char *names[KID_COUNT] = {"k_unpack", "k_residual", "k_passA", "k_passB", "k_maxdiag", "k_frame_inv", "k_schur",
                                           "k_ldl_diag", "k_ldl_trsm", "k_ldl_update", "k_ldl_backsolve", "k_backsub",
                                           "k_reduce_scalars", "k_ldl_panel", "k_pcg", "k_spcg", "k_spcg_pre", "k_prior"};
    return (kid >= 0 && kid < KID_COUNT) ? names[kid] : "?";
}

int aar_problem_pcg_iterations(aar_problem *pb, int32_t out[2]) {
    if (!pb || !out) return set_error(AAR_ERR_INVALID, "aar_problem_pcg_iterations: null argument");
    out[0] = out[1] = 0;
    if (!pb->P.use_pcg && !pb->P.use_spcg) return AAR_OK;
    HIP_TRY(hipSetDevice(pb->device));
    { int rc = copy_d2h(pb, out, pb->P.use_pcg ? pb->P.pcg_counter + 2 : pb->P.spcg_iters, 2 * sizeof(int32_t)); if (rc) return rc; }
    if (out[0] > SPCG_MAX_IT && pb->P.use_spcg) out[0] = SPCG_MAX_IT;   // (a timed-out launch records SPCG_BUFS)
    return AAR_OK;
}

int aar_problem_get_solver_stats(aar_problem *pb, aar_solver_stats *out) {
    if (!pb || !out) return set_error(AAR_ERR_INVALID, "aar_problem_get_solver_stats: null argument");
    // the caller says how large ITS struct is (a caller built against an older header has a shorter one): never write beyond it
    const size_t cap = out->struct_size;
    if (cap < 4 * sizeof(int32_t) || cap > 4096) return set_error(AAR_ERR_INVALID, "aar_solver_stats.struct_size is not set (sizeof(aar_solver_stats) of the caller)");
    aar_solver_stats st;
    memset(&st, 0, sizeof st);
    st.solver = pb->solver;
    st.deterministic = pb->P.deterministic;
    st.pcg_eta = pb->P.pcg_eta;
    st.pcg_max_it = pb->P.use_spcg ? pb->P.spcg_max_it : pb->P.pcg_max_it;
    st.pcg_eta_loose = pb->P.pcg_eta_loose;
    st.pcg_eta_switch = pb->P.pcg_eta_switch;
    st.pcg_abs_tol = pb->P.pcg_abs_tol;
    st.env_overrides = pb->env_overrides;
    st.fallbacks = pb->spcg_fallbacks;
    if (pb->P.use_pcg || pb->P.use_spcg) {
        int32_t c[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        HIP_TRY(hipSetDevice(pb->device));
        int rc = copy_d2h(pb, c, pb->P.use_spcg ? pb->P.spcg_iters : pb->P.pcg_counter + 2, (pb->P.use_spcg ? 8 : 3) * sizeof(int32_t));
        if (rc) return rc;
        st.last_iterations = std::min(c[0], pb->P.use_spcg ? SPCG_MAX_IT : c[0]);
        st.total_iterations = c[1];
        st.solves = c[2];
        st.same_xcd_solves = c[4];
    }
    st.struct_size = (uint32_t)std::min(cap, sizeof st);
    memcpy(out, &st, std::min(cap, sizeof st));
    return AAR_OK;
}

int aar_problem_set_test_hook(aar_problem *pb, int32_t hook, int32_t value) {
    if (!pb) return set_error(AAR_ERR_INVALID, "aar_problem_set_test_hook: null argument");
    if (hook == AAR_TEST_HOOK_SPCG_DROP) { pb->P.spcg_test_drop = value; return AAR_OK; }
    return set_error(AAR_ERR_INVALID, "aar_problem_set_test_hook: unknown hook %d", hook);
}

int aar_set_stage_timers(aar_problem *pb, int on) {
    if (!pb) return set_error(AAR_ERR_INVALID, "aar_set_stage_timers: null argument");
    HIP_TRY(hipSetDevice(pb->device));
    HIP_TRY(hipStreamSynchronize(pb->stream));
    pb->stage_timers = on != 0;
    memset(&pb->times, 0, sizeof pb->times);
    return AAR_OK;
}

int aar_get_stage_times(aar_problem *pb, aar_stage_times *t) {
    if (!pb || !t) return set_error(AAR_ERR_INVALID, "aar_get_stage_times: null argument");
    *t = pb->times;
    return AAR_OK;
}


// ------------------------------------------------------------------------------------------------
// Live tracker (live_kernels.hip): one frame per push, the window's LM in one launch
// ------------------------------------------------------------------------------------------------
struct aar_tracker {
    aar_tracker_params prm;
    aar_lm_params lm;
    int C = 0, M = 0, device = 0;
    hipStream_t stream = nullptr;
    double *d_ent = nullptr, *d_K = nullptr;
    double *d_state = nullptr;       // zslot [16][6] | anchor [6] + 2 idle | Ef [16] | Pe [16] | result record
    char *d_ring = nullptr;          // [lag + 1] slots
    char *h_stage = nullptr;         // pinned: one slot
    double *h_res = nullptr;         // pinned: the result record | start record | uncertainty record
    // marginalised anchor and covariance: what the last accepted push left
    bool unc_set = false;            // h_res holds the uncertainty record of push n - 1
    int has_marginal = 0;            // the next push puts the device's (Lambda_m, m) on its first window frame
    int64_t marginal_dropped = 0;
    int unc_W = 0;
    double unc_sigma2 = 0;
    size_t slot_bytes = 0;
    double half_size = 0;
    int64_t n = 0;                   // pushes accepted
    double times[LIVE_MAX_W];        // by ring slot
    int cnt[LIVE_MAX_W];
    // pushes of raw detections (aar_tracker_enable_detections)
    std::vector<double> sol_x, sol_K, sol_dist;   // the solution's camera | marker poses, cam_mats, dist_coeffs (zeros when it has none)
    int rc = 0, rm = 0;
    double marker_size = 0;
    bool det_on = false;
    aar_tracker_detection_params det;
    void *d_cams = nullptr;          // [C] CamTab
    double *d_toroot = nullptr;      // [C][12] | [M][12]
    double *d_work = nullptr;        // poses | Tc | BJ | cost, then has2 | fin (ints): sized by max_obs_per_frame, allocated once
    std::vector<int32_t> order;      // scratch of the candidate order
    // the gate (aar_tracker_enable_gate): a gated push refines through k_live_push_bank with this one-row member table,
    // which reads the kept count the gate kernel left in the slot header
    bool gate_on = false, gate_set = false;   // gate_set: gate_rec is the record of the last accepted push
    aar_tracker_gate_params gate;
    double gate_rec[LIVE_GATE_DOUBLES];
    double *h_back = nullptr;        // pinned: the gate record in front of h_res (one allocation, one copy back)
    LiveMember *d_gtab = nullptr;    // [1]
    double *d_gerr = nullptr;        // [max_obs_per_frame] e_d of the newest frame, then its keep flags (bytes)
    // constant-velocity motion model (aar_tracker_enable_motion): its pushes leave their records in a block of their own,
    // motion record | result | start record | uncertainty record, copied back in one piece; h_res then points into h_mot
    bool motion_called = false, motion_on = false, motion_set = false;   // motion_set: the fields below are those of the last accepted push
    aar_tracker_motion_params motion;
    MotionState mstate;              // the two newest estimates and their times
    double rel_slot[LIVE_MAX_W][6];  // by ring slot: the expected motion of the pair that ends at the frame
    double last_rel[6];
    int last_predicted = 0;
    double *d_mot = nullptr, *h_mot = nullptr;
};

namespace {

constexpr int LIVE_ST_ANCHOR = 6 * LIVE_MAX_W, LIVE_ST_EF = LIVE_ST_ANCHOR + 8, LIVE_ST_PE = LIVE_ST_EF + LIVE_MAX_W,
              LIVE_ST_GATE = LIVE_ST_PE + LIVE_MAX_W, LIVE_ST_RES = LIVE_ST_GATE + LIVE_GATE_DOUBLES,   // (the gate record rides in FRONT of the result)
              LIVE_ST_INFO = LIVE_ST_RES + LIVE_RES_DOUBLES, LIVE_ST_UNC = LIVE_ST_INFO + LIVE_INFO_DOUBLES,
              LIVE_ST_DOUBLES = LIVE_ST_UNC + LIVE_UNC_DOUBLES;   // (the info and uncertainty records ride behind the result: one copy)
constexpr int LIVE_DET_MAX_OBS = 4096;   // the vote is n^2 in ONE workgroup: a frame of raw detections is capped here

// the caller's struct read up to its struct_size, the rest at the defaults; false: too short to hold lag and smooth
void live_solution_z(const aar_dataset *sol, std::vector<double> &z);   // (below, with what a tracker and a bank member share)

bool tracker_params_read(const aar_tracker_params *in, aar_tracker_params *out) {
    aar_tracker_default_params(out);
    if (in->struct_size < offsetof(aar_tracker_params, smooth) + sizeof(int32_t)) return false;
    memcpy(out, in, std::min<size_t>(in->struct_size, sizeof *out));
    out->struct_size = (uint32_t)sizeof *out;
    return true;
}

}  // namespace

void aar_tracker_default_params(aar_tracker_params *p) {
    if (!p) return;
    memset(p, 0, sizeof *p);
    p->struct_size = (uint32_t)sizeof *p;
    p->huber_delta = 2.5f;
    p->max_obs_per_frame = 256;
}

int aar_tracker_params_validate(const aar_dataset *sol, const aar_tracker_params *in) {
    if (!sol || !in) return set_error(AAR_ERR_INVALID, "aar_tracker_params_validate: null argument");
    aar_tracker_params p;
    if (!tracker_params_read(in, &p)) return set_error(AAR_ERR_INVALID, "aar_tracker_params: struct_size %u does not reach lag / smooth", (unsigned)in->struct_size);
    if (p.lag < 0 || p.lag > AAR_TRACKER_MAX_LAG) return set_error(AAR_ERR_INVALID, "aar_tracker_params: lag = %d is outside 0 .. %d", (int)p.lag, AAR_TRACKER_MAX_LAG);
    if (p.smooth != 0 && p.smooth != 1) return set_error(AAR_ERR_INVALID, "aar_tracker_params: smooth = %d must be 0 or 1", (int)p.smooth);
    if (!p.smooth && p.lag > 0) return set_error(AAR_ERR_INVALID, "aar_tracker_params: lag = %d needs smooth = 1 (without a prior every frame stands alone)", (int)p.lag);
    if (p.smooth) {
        if (!(p.sigma_rot > 0.0) || !std::isfinite(p.sigma_rot)) return set_error(AAR_ERR_INVALID, "aar_tracker_params: sigma_rot = %g must be positive and finite", p.sigma_rot);
        if (!(p.sigma_trans > 0.0) || !std::isfinite(p.sigma_trans)) return set_error(AAR_ERR_INVALID, "aar_tracker_params: sigma_trans = %g must be positive and finite", p.sigma_trans);
    }
    if (p.with_huber && (!(p.huber_delta > 0.f) || !std::isfinite(p.huber_delta)))
        return set_error(AAR_ERR_INVALID, "aar_tracker_params: huber_delta = %g must be positive and finite", (double)p.huber_delta);
    if (p.max_obs_per_frame < 1 || p.max_obs_per_frame > (1 << 20))
        return set_error(AAR_ERR_INVALID, "aar_tracker_params: max_obs_per_frame = %d is outside 1 .. %d", (int)p.max_obs_per_frame, 1 << 20);
    if (p.anchor_mode != AAR_TRACKER_ANCHOR_FIXED && p.anchor_mode != AAR_TRACKER_ANCHOR_MARGINAL)
        return set_error(AAR_ERR_INVALID, "aar_tracker_params: anchor_mode = %d is neither AAR_TRACKER_ANCHOR_FIXED nor AAR_TRACKER_ANCHOR_MARGINAL",
                         (int)p.anchor_mode);
    if (p.anchor_mode == AAR_TRACKER_ANCHOR_MARGINAL && !p.smooth)
        return set_error(AAR_ERR_INVALID, "aar_tracker_params: anchor_mode = AAR_TRACKER_ANCHOR_MARGINAL needs smooth = 1 (the marginal is the prior's)");
    if (p.anchor_mode == AAR_TRACKER_ANCHOR_MARGINAL && p.lag < 1)
        return set_error(AAR_ERR_INVALID, "aar_tracker_params: anchor_mode = AAR_TRACKER_ANCHOR_MARGINAL needs lag >= 1 (with lag = 0 the next pair's "
                                          "time step is not known when the frame leaves)");
    if (p.covariance != 0 && p.covariance != 1) return set_error(AAR_ERR_INVALID, "aar_tracker_params: covariance = %d must be 0 or 1", (int)p.covariance);
    const int C = sol->num_cams, M = sol->num_markers;
    if (C < 1 || M < 1 || (int64_t)C + M >= 32768) return set_error(AAR_ERR_INVALID, "aar_tracker: solution with %d cameras / %d markers", C, M);
    if (sol->root_cam < 0 || sol->root_cam >= C || sol->root_marker < 0 || sol->root_marker >= M)
        return set_error(AAR_ERR_INVALID, "aar_tracker: solution root_cam = %d / root_marker = %d out of range", (int)sol->root_cam, (int)sol->root_marker);
    if (!sol->cam_mats || (C + M > 2 && !sol->x_full)) return set_error(AAR_ERR_INVALID, "aar_tracker: solution without cam_mats / x_full");
    if (!(sol->marker_size > 0.0) || !std::isfinite(sol->marker_size)) return set_error(AAR_ERR_INVALID, "aar_tracker: solution marker_size = %g must be positive and finite", sol->marker_size);
    for (int i = 0; i < 9 * C; i++)
        if (!std::isfinite(sol->cam_mats[i])) return set_error(AAR_ERR_INVALID, "aar_tracker: solution cam_mats[%d][%d] is not finite", i / 9, i % 9);
    for (int i = 0; i < 6 * (C - 1) + 6 * (M - 1); i++)
        if (!std::isfinite(sol->x_full[i])) return set_error(AAR_ERR_INVALID, "aar_tracker: solution x_full[%d] (a camera / marker pose) is not finite", i);
    return AAR_OK;
}

void aar_tracker_destroy(aar_tracker *t) {
    if (!t) return;
    (void)hipSetDevice(t->device);
    if (t->stream) (void)hipStreamSynchronize(t->stream);
    if (t->d_ent) (void)hipFree(t->d_ent);
    if (t->d_K) (void)hipFree(t->d_K);
    if (t->d_state) (void)hipFree(t->d_state);
    if (t->d_ring) (void)hipFree(t->d_ring);
    if (t->d_cams) (void)hipFree(t->d_cams);
    if (t->d_toroot) (void)hipFree(t->d_toroot);
    if (t->d_work) (void)hipFree(t->d_work);
    if (t->h_stage) (void)hipHostFree(t->h_stage);
    if (t->h_back) (void)hipHostFree(t->h_back);
    if (t->d_gtab) (void)hipFree(t->d_gtab);
    if (t->d_gerr) (void)hipFree(t->d_gerr);
    if (t->d_mot) (void)hipFree(t->d_mot);
    if (t->h_mot) (void)hipHostFree(t->h_mot);
    if (t->stream) (void)hipStreamDestroy(t->stream);
    delete t;
}

int aar_tracker_create(const aar_dataset *sol, const aar_tracker_params *in, const aar_lm_params *lm, aar_tracker **out) {
    if (!sol || !in || !out) return set_error(AAR_ERR_INVALID, "aar_tracker_create: null argument");
    *out = nullptr;
    int rc = aar_tracker_params_validate(sol, in);
    if (rc) return rc;
    aar_tracker_params p;
    (void)tracker_params_read(in, &p);
    if ((rc = ensure_device(p.device_id))) return rc;
    aar_tracker *t = new aar_tracker();
    t->prm = p;
    if (lm) t->lm = *lm; else aar_lm_default_params(&t->lm);
    t->C = sol->num_cams; t->M = sol->num_markers; t->device = p.device_id;
    t->half_size = (double)((float)sol->marker_size / 2.f);
    t->rc = sol->root_cam; t->rm = sol->root_marker; t->marker_size = sol->marker_size;
    if (sol->x_full) t->sol_x.assign(sol->x_full, sol->x_full + 6 * (size_t)(sol->num_cams - 1 + sol->num_markers - 1));
    t->sol_K.assign(sol->cam_mats, sol->cam_mats + 9 * (size_t)sol->num_cams);
    t->sol_dist.assign(5 * (size_t)sol->num_cams, 0.0);
    if (sol->dist_coeffs) t->sol_dist.assign(sol->dist_coeffs, sol->dist_coeffs + 5 * (size_t)sol->num_cams);
    t->slot_bytes = live_slot_bytes(p.max_obs_per_frame);
    const int C = t->C, M = t->M, A = C + M;
    double *d_z = nullptr;
    auto fail = [&](int code) { if (d_z) (void)hipFree(d_z); aar_tracker_destroy(t); return code; };
    if (hipStreamCreateWithFlags(&t->stream, hipStreamNonBlocking) != hipSuccess) return fail(set_error(AAR_ERR_HIP, "hipStreamCreate failed"));
    if (hipMalloc((void **)&t->d_ent, (size_t)A * ENT_STRIDE * sizeof(double)) != hipSuccess || hipMalloc((void **)&t->d_K, (size_t)9 * C * sizeof(double)) != hipSuccess ||
        hipMalloc((void **)&t->d_state, LIVE_ST_DOUBLES * sizeof(double)) != hipSuccess || hipMalloc((void **)&t->d_ring, (size_t)(p.lag + 1) * t->slot_bytes) != hipSuccess ||
        hipMalloc((void **)&d_z, (size_t)6 * A * sizeof(double)) != hipSuccess)
        return fail(set_error(AAR_ERR_HIP, "aar_tracker_create: hipMalloc failed"));
    if (hipHostMalloc((void **)&t->h_stage, t->slot_bytes, hipHostMallocDefault) != hipSuccess ||
        hipHostMalloc((void **)&t->h_back, (LIVE_GATE_DOUBLES + LIVE_RES_DOUBLES + LIVE_INFO_DOUBLES + LIVE_UNC_DOUBLES) * sizeof(double),
                      hipHostMallocDefault) != hipSuccess)
        return fail(set_error(AAR_ERR_HIP, "aar_tracker_create: hipHostMalloc failed"));
    t->h_res = t->h_back + LIVE_GATE_DOUBLES;
    if (hipMemsetAsync(t->d_state, 0, LIVE_ST_DOUBLES * sizeof(double), t->stream) != hipSuccess ||
        hipMemsetAsync(t->d_ring, 0, (size_t)(p.lag + 1) * t->slot_bytes, t->stream) != hipSuccess)
        return fail(set_error(AAR_ERR_HIP, "aar_tracker_create: hipMemset failed"));
    // the entity rows of the fixed cameras and markers, by the problem's own unpack kernel (roots: the identity)
    std::vector<double> z;
    live_solution_z(sol, z);
    const char *what = "";
    if (h2d(d_z, z.data(), z.size() * sizeof(double), t->stream, &what) || h2d(t->d_K, sol->cam_mats, (size_t)9 * C * sizeof(double), t->stream, &what))
        return fail(set_error(AAR_ERR_HIP, "aar_tracker_create: %s failed", what));
    DeviceProblem P;
    P.C = C; P.M = M; P.A = A; P.F = 0; P.intr = 0;
    P.z[0] = d_z; P.ent[0] = t->d_ent;
    launch_unpack(P, 0, t->stream);
    if (hipStreamSynchronize(t->stream) != hipSuccess) return fail(set_error(AAR_ERR_HIP, "aar_tracker_create: the unpack launch failed"));
    (void)hipFree(d_z);
    d_z = nullptr;
    if ((rc = check_async("tracker creation"))) return fail(rc);
    *out = t;
    return AAR_OK;
}

int aar_tracker_reset(aar_tracker *t) {
    if (!t) return set_error(AAR_ERR_INVALID, "aar_tracker_reset: null argument");
    t->n = 0;
    t->det_on = false;   // (the buffers stay; aar_tracker_enable_detections fills them again)
    t->gate_on = false;  // (likewise aar_tracker_enable_gate)
    t->gate_set = false;
    t->motion_called = t->motion_on = t->motion_set = false;   // (likewise aar_tracker_enable_motion)
    t->mstate = MotionState();
    t->h_res = t->h_back + LIVE_GATE_DOUBLES;   // (d_gtab's row may still point into d_mot: it is read only while gate_on, and
                                                // aar_tracker_enable_gate writes it again)
    t->unc_set = false;  // (the device's marginal stays where it is: no push reads it while has_marginal is 0)
    t->has_marginal = 0;
    t->marginal_dropped = 0;
    return AAR_OK;
}

namespace {

// ---- what a single tracker and a member of a tracker bank share; who: "" or "member b: " ----

// the rows of the fixed cameras and markers of a solution as the unpack kernel reads them: [C + M][6], the roots zero (the identity)
void live_solution_z(const aar_dataset *sol, std::vector<double> &z) {
    const int C = sol->num_cams, M = sol->num_markers;
    PoseLayout L;
    L.C = C; L.M = M; L.F = 0; L.rc = sol->root_cam; L.rm = sol->root_marker;
    const size_t at = z.size();
    z.resize(at + (size_t)6 * (C + M), 0.0);
    for (int c = 0; c < C; c++)
        if (c != L.rc) memcpy(&z[at + 6 * (size_t)c], sol->x_full + L.full_cam0() + 6LL * L.cam_slot(c), 6 * sizeof(double));
    for (int m = 0; m < M; m++)
        if (m != L.rm) memcpy(&z[at + 6 * (size_t)(C + m)], sol->x_full + L.full_mk0() + 6LL * L.mk_slot(m), 6 * sizeof(double));
}

// one frame's detections against the tracker's sizes
int live_check_frame(const char *fn, const char *who, bool raw, int C, int M, int max_obs, int32_t n_obs, const int32_t *obs_cam,
                     const int32_t *obs_marker, const float *obs_uv) {
    if (n_obs < 0 || n_obs > max_obs)
        return set_error(AAR_ERR_INVALID, "%s: %s%s = %d is outside 0 .. max_obs_per_frame = %d", fn, who, raw ? "n_det" : "n_obs", (int)n_obs, max_obs);
    if (n_obs > 0 && (!obs_cam || !obs_marker || !obs_uv)) return set_error(AAR_ERR_INVALID, "%s: %snull %s array", fn, who, raw ? "detection" : "observation");
    for (int o = 0; o < n_obs; o++) {
        if (obs_cam[o] < 0 || obs_cam[o] >= C)
            return set_error(AAR_ERR_INVALID, "%s: %s%s[%d] = %d is outside 0 .. %d", fn, who, raw ? "det_cam" : "obs_cam", o, (int)obs_cam[o], C - 1);
        if (obs_marker[o] < 0 || obs_marker[o] >= M)
            return set_error(AAR_ERR_INVALID, "%s: %s%s[%d] = %d is outside 0 .. %d", fn, who, raw ? "det_marker" : "obs_marker", o, (int)obs_marker[o], M - 1);
    }
    return AAR_OK;
}

int live_check_pose_init(const char *fn, const char *who, const double *pose_init) {
    for (int k = 0; pose_init && k < 6; k++)
        if (!std::isfinite(pose_init[k])) return set_error(AAR_ERR_INVALID, "%s: %spose_init[%d] is not finite", fn, who, k);
    return AAR_OK;
}

// a vote is held unless the caller's pose_init settles the start (policy VOTE) or the frame has too few detections
bool live_do_vote(const aar_tracker_detection_params &det, int32_t n_obs, bool has_init) {
    return n_obs >= det.min_detections && !(has_init && det.start_policy == AAR_TRACKER_START_VOTE);
}

// the frame's slot: header | records (| on a push of raw detections the candidate order), staged in page-locked memory; returns its bytes
size_t live_stage_slot(char *slot, int C, bool raw, int32_t n_obs, const int32_t *obs_cam, const int32_t *obs_marker, const float *obs_uv,
                       const double *pose_init, std::vector<int32_t> &order) {
    double *hdr = reinterpret_cast<double *>(slot);
    for (int k = 0; k < 8; k++) hdr[k] = (pose_init && k < 6) ? pose_init[k] : 0.0;
    for (int o = 0; o < n_obs; o++) {
        char *rec = slot + LIVE_HDR_BYTES + (size_t)LIVE_REC_BYTES * o;
        ObsIdx id;
        id.frame = 0; id.cam = obs_cam[o]; id.marker = C + obs_marker[o]; id.slots = 0;
        memcpy(rec, &id, sizeof id);
        memcpy(rec + sizeof id, obs_uv + 8 * (size_t)o, 8 * sizeof(float));
    }
    size_t bytes = LIVE_HDR_BYTES + (size_t)LIVE_REC_BYTES * n_obs;
    if (raw) {
        // the candidate order of init_object_transforms: marker, then camera, stable (host/initializer.cpp); behind the records, same copy
        order.resize((size_t)n_obs);
        for (int o = 0; o < n_obs; o++) order[o] = o;
        std::stable_sort(order.begin(), order.end(), [&](int32_t x, int32_t y) {
            return obs_marker[x] != obs_marker[y] ? obs_marker[x] < obs_marker[y] : obs_cam[x] < obs_cam[y];
        });
        if (n_obs) memcpy(slot + bytes, order.data(), sizeof(int32_t) * (size_t)n_obs);
        bytes += sizeof(int32_t) * (size_t)n_obs;
    }
    return bytes;
}

// what push n (n pushes accepted before it) at frame_time gives every tracker with these parameters: the LM's settings, the window in the ring,
// the pair weights from the times by ring slot.  cnt is zeroed; ent .. res, has_init, has_marginal, rows and unc are the caller's.
void live_window_args(LiveArgs &a, const aar_tracker_params &p, const aar_lm_params &lm, int64_t n, double frame_time, const double *times) {
    const int slots = p.lag + 1, ns = (int)(n % slots);
    const int W = (int)std::min<int64_t>(n + 1, slots);
    const bool has_anchor = n - slots >= 0;
    a.huber = p.with_huber ? p.huber_delta : -1.f;
    a.max_iters = lm.max_iters; a.min_error = lm.min_error; a.min_step_error_diff = lm.min_step_error_diff;
    a.min_average_step_error_diff = lm.min_average_step_error_diff; a.tau = lm.tau;
    a.W = W; a.slots = slots; a.first_slot = (int)((n + 1 - W) % slots);
    a.has_anchor = has_anchor ? 1 : 0; a.smooth = p.smooth;
    for (int i = 0; i < LIVE_MAX_W; i++) { a.cnt[i] = 0; a.lam[i][0] = a.lam[i][1] = 0.0; }
    for (int i = 0; i < W; i++) {
        const int sl = (a.first_slot + i) % slots;
        const double ti = i == W - 1 ? frame_time : times[sl];
        double tp = 0.0;
        bool pair = false;
        if (i > 0) { tp = times[(a.first_slot + i - 1) % slots]; pair = true; }
        else if (has_anchor) { tp = times[ns]; pair = true; }   // the anchor's time still sits in the slot the new frame takes
        if (pair && p.smooth) {
            const double dt = ti - tp;
            a.lam[i][0] = 1.0 / (p.sigma_rot * p.sigma_rot * dt);
            a.lam[i][1] = 1.0 / (p.sigma_trans * p.sigma_trans * dt);
        }
    }
    const bool marginal = p.anchor_mode == AAR_TRACKER_ANCHOR_MARGINAL;
    a.anchor_pair = has_anchor && !marginal ? 1 : 0;
    a.marginal = marginal ? 1 : 0; a.covariance = p.covariance;
}

// 8 rows per detection of the window, 6 per pair; the anchor pair's 6 are the marginal prior's in that mode (none after a dropped marginal)
double live_rows(const LiveArgs &a, int64_t det, int has_marginal) {
    return 8.0 * (double)det + (a.smooth ? 6.0 * (double)(a.W - 1 + (a.marginal ? has_marginal : a.has_anchor ? 1 : 0)) : 0.0);
}

double live_sigma2(double rows, int W, double final_cost) {
    const double dof = rows - 6.0 * (double)W;
    return dof > 0.0 ? final_cost / dof : 0.0;
}

// the device's result record h of push n -> the caller's struct
void live_fill_result(const double *h, int64_t n, int W, int slots, std::chrono::steady_clock::time_point t0, aar_tracker_result *result) {
    aar_tracker_result r;
    memset(&r, 0, sizeof r);
    r.struct_size = result->struct_size;
    r.frame_index = n; r.window_frames = W;
    r.iterations = (int32_t)h[0]; r.stop_code = (int32_t)h[1]; r.rejected_tries = (int32_t)h[2];
    r.initial_cost = h[3]; r.final_cost = h[4]; r.final_data_cost = h[5]; r.final_prior_cost = h[6]; r.final_mu = h[7];
    for (int k = 0; k < 6; k++) { r.pose[k] = h[8 + k]; r.lagged_pose[k] = W == slots ? h[14 + k] : 0.0; }
    r.has_lagged = W == slots ? 1 : 0;
    r.lagged_index = W == slots ? n + 1 - W : -1;
    r.seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    memcpy(result, &r, std::min<size_t>(result->struct_size, sizeof r));
}

void live_fill_info(const double *h_info, aar_tracker_start_info *info) {
    aar_tracker_start_info si;
    memset(&si, 0, sizeof si);
    si.struct_size = (uint32_t)std::min<size_t>(info->struct_size, sizeof si);
    si.voted = (int32_t)h_info[0]; si.candidates = (int32_t)h_info[1]; si.winner = (int32_t)h_info[2]; si.vote_cost = h_info[3];
    si.start_source = (int32_t)h_info[4]; si.cost_prediction = h_info[5]; si.cost_vote = h_info[6];
    for (int k = 0; k < 6; k++) si.start_pose[k] = h_info[8 + k];
    memcpy(info, &si, si.struct_size);
}

// the host copy u of the device's uncertainty record after push n - 1 -> the caller's struct
void live_fill_uncertainty(const aar_tracker_params &prm, const double *u, int W, int64_t n, int has_marginal, int64_t marginal_dropped, double sigma2,
                           aar_tracker_uncertainty_record *out) {
    aar_tracker_uncertainty_record r;
    memset(&r, 0, sizeof r);
    r.struct_size = out->struct_size;
    r.cov_valid = prm.covariance && u[LIVE_UNC_VALID] != 0.0 ? 1 : 0;
    r.sigma2 = prm.covariance ? sigma2 : 0.0;
    r.window_frames = W;
    for (int i = 0; i < W; i++) r.frame_index[i] = n - W + i;
    if (r.cov_valid) memcpy(r.cov, u + LIVE_UNC_HDR, 36 * (size_t)W * sizeof(double));
    r.has_marginal = has_marginal;
    r.marginal_index = has_marginal ? n - W + 1 : -1;
    if (has_marginal) {
        memcpy(r.marginal_info, u + LIVE_UNC_LM, 36 * sizeof(double));
        memcpy(r.marginal_mean, u + LIVE_UNC_M, 6 * sizeof(double));
    }
    r.marginal_dropped = marginal_dropped;
    memcpy(out, &r, std::min<size_t>(out->struct_size, sizeof r));
}

// aar_tracker_window's outputs from a tracker's state st [LIVE_ST_RES] after n pushes; without st only the counts
void live_window_out(const double *st, int64_t n, int slots, int32_t *n_out, int64_t *frame_index, double *poses, double *frame_err, double *pair_err,
                     double anchor_pose[6], int32_t *has_anchor) {
    const int W = (int)std::min<int64_t>(n, slots);
    const bool anchored = n - 1 - slots >= 0;
    if (n_out) *n_out = W;
    if (has_anchor) *has_anchor = anchored ? 1 : 0;
    if (frame_index) for (int i = 0; i < W; i++) frame_index[i] = n - W + i;
    if (!st) return;
    for (int i = 0; i < W; i++) {
        const int sl = (int)((n - W + i) % slots);
        if (poses) memcpy(poses + 6 * (size_t)i, st + 6 * sl, 6 * sizeof(double));
        if (frame_err) frame_err[i] = st[LIVE_ST_EF + i];
        if (pair_err) pair_err[i] = st[LIVE_ST_PE + i];
    }
    if (anchor_pose) for (int k = 0; k < 6; k++) anchor_pose[k] = anchored ? st[LIVE_ST_ANCHOR + k] : 0.0;
}

// the tables k_live_init reads: K and twelve coefficients by camera index (CamTab); the to-root 3x4 of every camera and marker exactly as
// aar_initializer_object_poses builds them from the solution (host cv::Rodrigues), the identity for the roots
void live_detection_tables(int C, int M, int rc, int rm, const aar_cam_model *cams, const double *sol_x, const double *sol_K, const double *sol_dist,
                           double *tab, double *tr) {
    for (int c = 0; c < C; c++) {
        double *row = tab + (size_t)c * (9 + AAR_MAX_DIST);
        for (int i = 0; i < 9 + AAR_MAX_DIST; i++) row[i] = 0.0;
        if (cams) {
            memcpy(row, cams[c].K, 9 * sizeof(double));
            for (int i = 0; i < cams[c].n_dist; i++) row[9 + i] = cams[c].dist[i];
        } else {
            memcpy(row, sol_K + 9 * (size_t)c, 9 * sizeof(double));
            memcpy(row + 9, sol_dist + 5 * (size_t)c, 5 * sizeof(double));
        }
    }
    PoseLayout L;
    L.C = C; L.M = M; L.F = 0; L.rc = rc; L.rm = rm;
    for (int e = 0; e < C + M; e++) {
        double *m = tr + 12 * (size_t)e;
        for (int i = 0; i < 12; i++) m[i] = 0.0;
        m[0] = m[5] = m[10] = 1.0;
        const bool cam = e < C;
        if (cam ? e == L.rc : e - C == L.rm) continue;
        const double *v = sol_x + (cam ? L.full_cam0() + 6LL * L.cam_slot(e) : L.full_mk0() + 6LL * L.mk_slot(e - C));
        const Rigid r = pose_to_rigid(v);
        for (int i = 0; i < 3; i++) {
            for (int j = 0; j < 3; j++) m[i * 4 + j] = r.R[i * 3 + j];
            m[i * 4 + 3] = r.t[i];
        }
    }
}

// one push.  info == nullptr && !raw: aar_tracker_push (corners already undistorted, ONE launch).  raw: aar_tracker_push_detections -- the
// corners are raw, k_live_init undistorts them in the slot and chooses the start, then the same k_live_push runs from the slot's header.
int tracker_push(aar_tracker *t, const char *fn, bool raw, double frame_time, int32_t n_obs, const int32_t *obs_cam, const int32_t *obs_marker,
                 const float *obs_uv, const double *pose_init, aar_tracker_result *result, aar_tracker_start_info *info) {
    if (!t) return set_error(AAR_ERR_INVALID, "%s: null argument", fn);
    const auto t0 = std::chrono::steady_clock::now();
    const aar_tracker_params &p = t->prm;
    const int slots = p.lag + 1;
    const int64_t n = t->n;
    if (raw && !t->det_on) return set_error(AAR_ERR_INVALID, "%s: call aar_tracker_enable_detections first", fn);
    if (int rc = live_check_frame(fn, "", raw, t->C, t->M, p.max_obs_per_frame, n_obs, obs_cam, obs_marker, obs_uv)) return rc;
    if (!std::isfinite(frame_time)) return set_error(AAR_ERR_INVALID, "%s: frame_time is not finite", fn);
    const int ns = (int)(n % slots), ps = (int)((n + slots - 1) % slots);
    if (n > 0 && (!(frame_time > t->times[ps]) || !std::isfinite(frame_time - t->times[ps])))
        return set_error(AAR_ERR_INVALID, "%s: frame_time = %g does not ascend from the previous push's %g", fn, frame_time, t->times[ps]);
    const bool do_vote = raw && live_do_vote(t->det, n_obs, pose_init != nullptr);
    if (n == 0 && !pose_init && !raw) return set_error(AAR_ERR_INVALID, "%s: the first push needs a pose_init", fn);
    if (n == 0 && !pose_init && !do_vote)
        return set_error(AAR_ERR_INVALID, "%s: the first push has %d detections, fewer than min_detections = %d, and no pose_init: nothing to start from", fn,
                         (int)n_obs, (int)t->det.min_detections);
    if (int rc = live_check_pose_init(fn, "", pose_init)) return rc;
    HIP_TRY(hipSetDevice(t->device));
    const size_t copy_bytes = live_stage_slot(t->h_stage, t->C, raw, n_obs, obs_cam, obs_marker, obs_uv, pose_init, t->order);
    const bool gate = t->gate_on;
    if (gate) {   // as a bank member: the gate and the refinement read the frame's count and whether it brings a start from the header
        double *hdr = reinterpret_cast<double *>(t->h_stage);
        hdr[LIVE_HDR_CNT] = (double)n_obs;
        hdr[LIVE_HDR_INIT] = pose_init ? 1.0 : 0.0;
    }
    // the motion model: the expected motion of the new pair and the prediction, from the estimates the last accepted push left.  The prediction
    // rides in the slot header, where a caller's pose_init would be: a frame without one starts there
    const bool motion = t->motion_on;
    double rel_n[6] = {0, 0, 0, 0, 0, 0}, pred[6];
    bool predicted = false, start_pred = false;
    if (motion) {
        predicted = motion_measure(t->mstate, frame_time, t->motion.max_dt, rel_n, pred);
        if (!pose_init && n > 0) {
            double *hdr = reinterpret_cast<double *>(t->h_stage);
            memcpy(hdr, pred, sizeof pred);
            if (gate && !raw) hdr[LIVE_HDR_INIT] = 1.0;
            start_pred = true;
        }
    }
    // the records of a push, gate record | result | start record | uncertainty record: in the tracker's state, or behind the motion record in the
    // model's own block
    double *d_rec = motion ? t->d_mot + LIVE_MOT_DOUBLES : t->d_state + LIVE_ST_GATE;
    LiveArgs a;
    live_window_args(a, p, t->lm, n, frame_time, t->times);
    a.ent = t->d_ent; a.Kmat = t->d_K; a.ring = t->d_ring; a.slot_bytes = t->slot_bytes;
    a.zslot = t->d_state; a.anchor = t->d_state + LIVE_ST_ANCHOR; a.Ef = t->d_state + LIVE_ST_EF; a.Pe = t->d_state + LIVE_ST_PE; a.res = d_rec + LIVE_GATE_DOUBLES;
    a.h = t->half_size;
    a.has_init = (pose_init || raw || start_pred) ? 1 : 0;   // raw: k_live_init wrote the header
    const int W = a.W;
    int64_t det = 0;
    for (int i = 0; i < W; i++) {
        a.cnt[i] = i == W - 1 ? n_obs : t->cnt[(a.first_slot + i) % slots];
        det += a.cnt[i];
    }
    const bool marginal = a.marginal != 0, tail = marginal || p.covariance;
    a.has_marginal = marginal ? t->has_marginal : 0;
    a.unc = a.res + LIVE_RES_DOUBLES + LIVE_INFO_DOUBLES;
    a.rows = live_rows(a, det, a.has_marginal);
    double rel[LIVE_MAX_W][6];   // by window position
    if (motion) {
        memset(rel, 0, sizeof rel);
        memcpy(rel[W - 1], rel_n, sizeof rel_n);
        for (int i = 0; i + 1 < W; i++) memcpy(rel[i], t->rel_slot[(a.first_slot + i) % slots], sizeof rel[i]);
    }
    HIP_TRY(hipMemcpyAsync(t->d_ring + (size_t)ns * t->slot_bytes, t->h_stage, copy_bytes, hipMemcpyHostToDevice, t->stream));
    double *h_info = t->h_res + LIVE_RES_DOUBLES;
    if (raw) {
        const size_t mo = (size_t)p.max_obs_per_frame;
        LiveInitArgs li;
        li.slot = t->d_ring + (size_t)ns * t->slot_bytes; li.n_det = n_obs;
        li.cams = t->d_cams; li.Tcr = t->d_toroot; li.Tmr = t->d_toroot + 12 * (size_t)t->C; li.C = t->C;
        li.hf = (float)t->marker_size / 2.0f; li.h = t->marker_size / 2;   // as the Initializer: float for IPPE, double for the vote
        li.threshold = t->det.ippe_threshold;
        li.do_vote = do_vote ? 1 : 0; li.policy = t->det.start_policy; li.has_init = pose_init ? 1 : 0; li.has_prev = n > 0 ? 1 : 0;
        li.zprev = start_pred ? reinterpret_cast<const double *>(li.slot) : t->d_state + 6 * ps;   // (the kernel reads it before it writes the header)
        li.ent = t->d_ent; li.Kmat = t->d_K; li.huber = a.huber; li.h_track = t->half_size;
        live_init_work_carve(li, t->d_work, mo);
        li.info = a.res + LIVE_RES_DOUBLES;
        launch_live_init(li, t->stream);
        if (n == 0 && !pose_init) {
            // the only push a vote can fail with nothing to fall back on: read the info before the window is touched
            HIP_TRY(hipMemcpyAsync(h_info, li.info, LIVE_INFO_DOUBLES * sizeof(double), hipMemcpyDeviceToHost, t->stream));
            HIP_TRY(hipStreamSynchronize(t->stream));
            if (int rc = check_async("k_live_init")) return rc;
            if (h_info[4] < 0.0)
                return set_error(AAR_ERR_NUMERIC, "%s: no finite object pose candidate among %d, and neither a pose_init nor a previous estimate", fn, (int)h_info[1]);
        }
    }
    if (gate) {
        // the gate compacts the new slot and leaves the kept count in its header; the refinement is the bank's instance on a one-row table, which
        // reads every window frame's count from the headers (the earlier frames' were left there by their own pushes): no host wait in between
        LiveGateArgs ga;
        ga.slot = t->d_ring + (size_t)ns * t->slot_bytes; ga.n = n_obs; ga.has_init = a.has_init; ga.zprev = t->d_state + 6 * ps;
        ga.ent = t->d_ent; ga.Kmat = t->d_K; ga.h = t->half_size;
        ga.g.k_median = t->gate.k_median; ga.g.min_px = t->gate.min_px; ga.g.min_detections = t->gate.min_detections;
        ga.rec = d_rec; ga.det_err = t->d_gerr;
        ga.keep = reinterpret_cast<uint8_t *>(t->d_gerr + (size_t)p.max_obs_per_frame);
        launch_live_gate(ga, t->stream);
        LiveBankArgs ba;
        memset(&ba, 0, sizeof ba);
        ba.sh = a;
        ba.tab = t->d_gtab; ba.raw = raw ? 1 : 0; ba.fresh = n == 0 ? 1 : 0;
        if (motion) {
            LiveMemberMotionArgs gm;
            gm.ba = ba;
            memcpy(gm.rel, rel, sizeof rel);
            gm.mot = t->d_mot;
            launch_live_push_member_motion(gm, t->stream);
        } else {
            launch_live_push_bank(ba, 1, t->stream);
        }
    } else if (motion) {
        LiveMotionArgs ma;
        ma.a = a;
        memcpy(ma.rel, rel, sizeof rel);
        ma.mot = t->d_mot;
        launch_live_push_motion(ma, t->stream);
    } else {
        launch_live_push(a, t->stream);
    }
    // one copy: the result, the start record (also when the tail's record behind it is wanted) and the uncertainty record up to the window's blocks
    // (and, in front of the result, the gate record)
    const size_t back = tail ? LIVE_RES_DOUBLES + LIVE_INFO_DOUBLES + LIVE_UNC_HDR + (p.covariance ? 36 * (size_t)W : 0)
                             : LIVE_RES_DOUBLES + (raw ? LIVE_INFO_DOUBLES : 0);
    if (tail) t->unc_set = false;   // the copy overwrites the record aar_tracker_uncertainty serves: a push that fails from here on leaves none
    if (motion) HIP_TRY(hipMemcpyAsync(t->h_mot, t->d_mot, (LIVE_MOT_DOUBLES + LIVE_GATE_DOUBLES + back) * sizeof(double), hipMemcpyDeviceToHost, t->stream));
    else if (gate) HIP_TRY(hipMemcpyAsync(t->h_back, d_rec, (LIVE_GATE_DOUBLES + back) * sizeof(double), hipMemcpyDeviceToHost, t->stream));
    else HIP_TRY(hipMemcpyAsync(t->h_res, a.res, back * sizeof(double), hipMemcpyDeviceToHost, t->stream));
    HIP_TRY(hipStreamSynchronize(t->stream));
    int rc = check_async("k_live_push");
    if (rc) return rc;
    // the push is accepted: the frame that leaves the window hands its slot to the new one
    t->times[ns] = frame_time;
    t->cnt[ns] = n_obs;
    if (gate) {   // later pushes, the rows and sigma2 see the compacted frame
        memcpy(t->gate_rec, t->h_res - LIVE_GATE_DOUBLES, sizeof t->gate_rec);
        t->gate_set = true;
        t->cnt[ns] = (int)t->gate_rec[2];
        a.rows = live_rows(a, det - n_obs + t->cnt[ns], a.has_marginal);
    }
    t->n = n + 1;
    if (motion) {
        // the two newest estimates at this push's final point: the kernel's motion record and the result's newest pose
        MotionState &m = t->mstate;
        if (n > 0) { memcpy(m.za, t->h_mot, sizeof m.za); m.ta = m.tb; }
        memcpy(m.zb, t->h_res + 8, sizeof m.zb);
        m.tb = frame_time;
        m.frames = n > 0 ? 2 : 1;
        memcpy(t->rel_slot[ns], rel_n, sizeof t->rel_slot[ns]);
        memcpy(t->last_rel, rel_n, sizeof t->last_rel);
        t->last_predicted = predicted ? 1 : 0;
        t->motion_set = true;
        if (raw && start_pred && predicted && h_info[4] == 1.0) h_info[4] = 3.0;   // the "previous estimate" the start kernel chose was the motion prediction
    }
    if (tail) {
        const double *u = t->h_res + LIVE_RES_DOUBLES + LIVE_INFO_DOUBLES;
        t->unc_set = true;
        t->unc_W = W;
        t->has_marginal = marginal && u[LIVE_UNC_HAS] != 0.0 ? 1 : 0;
        if (marginal && u[LIVE_UNC_DROP] != 0.0) t->marginal_dropped++;
        t->unc_sigma2 = live_sigma2(a.rows, W, t->h_res[4]);
    }
    if (result) live_fill_result(t->h_res, n, W, slots, t0, result);
    if (info) live_fill_info(h_info, info);
    return AAR_OK;
}

// the caller's struct read up to its struct_size, the rest at the defaults; false: too short to hold start_policy
bool detection_params_read(const aar_tracker_detection_params *in, aar_tracker_detection_params *out) {
    aar_tracker_default_detection_params(out);
    if (in->struct_size < offsetof(aar_tracker_detection_params, start_policy) + sizeof(int32_t)) return false;
    memcpy(out, in, std::min<size_t>(in->struct_size, sizeof *out));
    out->struct_size = (uint32_t)sizeof *out;
    return true;
}

int detection_params_check(int C, const aar_tracker_detection_params *in, aar_tracker_detection_params *p) {
    if (!detection_params_read(in, p))
        return set_error(AAR_ERR_INVALID, "aar_tracker_detection_params: struct_size %u does not reach start_policy", (unsigned)in->struct_size);
    if (!(p->ippe_threshold > 0.0) || !std::isfinite(p->ippe_threshold))
        return set_error(AAR_ERR_INVALID, "aar_tracker_detection_params: ippe_threshold = %g must be positive and finite", p->ippe_threshold);
    if (p->min_detections < 1) return set_error(AAR_ERR_INVALID, "aar_tracker_detection_params: min_detections = %d must be at least 1", (int)p->min_detections);
    if (p->start_policy != AAR_TRACKER_START_VOTE && p->start_policy != AAR_TRACKER_START_BEST)
        return set_error(AAR_ERR_INVALID, "aar_tracker_detection_params: start_policy = %d is neither AAR_TRACKER_START_VOTE nor AAR_TRACKER_START_BEST",
                         (int)p->start_policy);
    for (int c = 0; p->cams && c < C; c++) {
        const aar_cam_model &m = p->cams[c];
        for (int i = 0; i < 9; i++)
            if (!std::isfinite(m.K[i])) return set_error(AAR_ERR_INVALID, "aar_tracker_detection_params: cams[%d].K[%d] is not finite", c, i);
        if (m.n_dist < 0 || m.n_dist > AAR_MAX_DIST)
            return set_error(AAR_ERR_INVALID, "aar_tracker_detection_params: cams[%d].n_dist = %d is outside 0 .. %d", c, (int)m.n_dist, AAR_MAX_DIST);
        for (int i = 0; i < m.n_dist; i++)
            if (!std::isfinite(m.dist[i])) return set_error(AAR_ERR_INVALID, "aar_tracker_detection_params: cams[%d].dist[%d] is not finite", c, i);
    }
    return AAR_OK;
}

}  // namespace

int aar_tracker_push(aar_tracker *t, double frame_time, int32_t n_obs, const int32_t *obs_cam, const int32_t *obs_marker, const float *obs_uv,
                     const double *pose_init, aar_tracker_result *result) {
    return tracker_push(t, "aar_tracker_push", false, frame_time, n_obs, obs_cam, obs_marker, obs_uv, pose_init, result, nullptr);
}

int aar_tracker_push_detections(aar_tracker *t, double frame_time, int32_t n_det, const int32_t *det_cam, const int32_t *det_marker,
                                const float *det_uv_raw, const double *pose_init, aar_tracker_result *result, aar_tracker_start_info *info) {
    return tracker_push(t, "aar_tracker_push_detections", true, frame_time, n_det, det_cam, det_marker, det_uv_raw, pose_init, result, info);
}

void aar_tracker_default_detection_params(aar_tracker_detection_params *p) {
    if (!p) return;
    memset(p, 0, sizeof *p);
    p->struct_size = (uint32_t)sizeof *p;
    p->ippe_threshold = 2.0;
    p->min_detections = 2;
    p->start_policy = AAR_TRACKER_START_VOTE;
}

int aar_tracker_detection_params_validate(const aar_dataset *sol, const aar_tracker_detection_params *in) {
    if (!sol || !in) return set_error(AAR_ERR_INVALID, "aar_tracker_detection_params_validate: null argument");
    if (sol->num_cams < 1) return set_error(AAR_ERR_INVALID, "aar_tracker_detection_params_validate: solution with %d cameras", (int)sol->num_cams);
    aar_tracker_detection_params p;
    return detection_params_check(sol->num_cams, in, &p);
}

int aar_tracker_enable_detections(aar_tracker *t, const aar_tracker_detection_params *in) {
    if (!in) return set_error(AAR_ERR_INVALID, "aar_tracker_enable_detections: null argument");
    if (!t) {   // no tracker exists without a device: say which of the two it is
        if (int rc = ensure_device(0)) return rc;
        return set_error(AAR_ERR_INVALID, "aar_tracker_enable_detections: null tracker");
    }
    if (t->det_on) return set_error(AAR_ERR_INVALID, "aar_tracker_enable_detections: already enabled (aar_tracker_reset first)");
    if (t->n != 0) return set_error(AAR_ERR_INVALID, "aar_tracker_enable_detections: call it after aar_tracker_create or aar_tracker_reset, before the first push");
    aar_tracker_detection_params p;
    if (int rc = detection_params_check(t->C, in, &p)) return rc;
    if (t->prm.max_obs_per_frame > LIVE_DET_MAX_OBS)
        return set_error(AAR_ERR_UNSUPPORTED, "aar_tracker_enable_detections: max_obs_per_frame = %d is above %d (the vote runs in one workgroup)",
                         (int)t->prm.max_obs_per_frame, LIVE_DET_MAX_OBS);
    HIP_TRY(hipSetDevice(t->device));
    const int C = t->C, M = t->M;
    const size_t mo = (size_t)t->prm.max_obs_per_frame;
    if (!t->d_cams) HIP_TRY(hipMalloc(&t->d_cams, (size_t)C * (9 + AAR_MAX_DIST) * sizeof(double)));
    if (!t->d_toroot) HIP_TRY(hipMalloc((void **)&t->d_toroot, 12 * (size_t)(C + M) * sizeof(double)));
    if (!t->d_work) HIP_TRY(hipMalloc((void **)&t->d_work, 98 * mo * sizeof(double) + 3 * mo * sizeof(int)));
    std::vector<double> tab((size_t)C * (9 + AAR_MAX_DIST), 0.0), tr(12 * (size_t)(C + M), 0.0);
    live_detection_tables(C, M, t->rc, t->rm, p.cams, t->sol_x.data(), t->sol_K.data(), t->sol_dist.data(), tab.data(), tr.data());
    const char *what = "";
    if (h2d(t->d_cams, tab.data(), tab.size() * sizeof(double), t->stream, &what) || h2d(t->d_toroot, tr.data(), tr.size() * sizeof(double), t->stream, &what))
        return set_error(AAR_ERR_HIP, "aar_tracker_enable_detections: %s failed", what);
    HIP_TRY(hipStreamSynchronize(t->stream));
    p.cams = nullptr;   // (copied; the caller's array is not kept)
    t->det = p;
    t->det_on = true;
    return AAR_OK;
}

int aar_tracker_uncertainty(aar_tracker *t, aar_tracker_uncertainty_record *out) {
    if (!t || !out) return set_error(AAR_ERR_INVALID, "aar_tracker_uncertainty: null argument");
    if (t->prm.anchor_mode == AAR_TRACKER_ANCHOR_FIXED && !t->prm.covariance)
        return set_error(AAR_ERR_INVALID, "aar_tracker_uncertainty: the tracker was created with anchor_mode fixed and covariance = 0: nothing is kept");
    if (!t->unc_set || t->n == 0) return set_error(AAR_ERR_INVALID, "aar_tracker_uncertainty: no push since creation / reset");
    if (out->struct_size < offsetof(aar_tracker_uncertainty_record, cov_valid) + sizeof(int32_t))
        return set_error(AAR_ERR_INVALID, "aar_tracker_uncertainty: struct_size %u does not reach cov_valid", (unsigned)out->struct_size);
    live_fill_uncertainty(t->prm, t->h_res + LIVE_RES_DOUBLES + LIVE_INFO_DOUBLES, t->unc_W, t->n, t->has_marginal, t->marginal_dropped, t->unc_sigma2, out);
    return AAR_OK;
}

int aar_tracker_window(aar_tracker *t, int32_t *n_out, int64_t *frame_index, double *poses, double *frame_err, double *pair_err, double anchor_pose[6],
                       int32_t *has_anchor) {
    if (!t) return set_error(AAR_ERR_INVALID, "aar_tracker_window: null argument");
    const int slots = t->prm.lag + 1;
    live_window_out(nullptr, t->n, slots, n_out, frame_index, poses, frame_err, pair_err, anchor_pose, has_anchor);
    if (t->n == 0 || (!poses && !frame_err && !pair_err && !anchor_pose)) return AAR_OK;
    HIP_TRY(hipSetDevice(t->device));
    double st[LIVE_ST_RES];
    const char *what = "";
    if (d2h(st, t->d_state, sizeof st, t->stream, &what)) return set_error(AAR_ERR_HIP, "aar_tracker_window: %s failed", what);
    live_window_out(st, t->n, slots, nullptr, nullptr, poses, frame_err, pair_err, anchor_pose, nullptr);
    return AAR_OK;
}

// ------------------------------------------------------------------------------------------------
// Tracker bank: B live trackers in lockstep, member b = workgroup b of one launch
// ------------------------------------------------------------------------------------------------
struct aar_tracker_bank {
    struct Member {
        int C = 0, M = 0, rc = 0, rm = 0;
        double marker_size = 0, half_size = 0;
        size_t ent0 = 0, cam0 = 0;       // its first entity row / camera in the bank's tables
        std::vector<double> sol_x, sol_K, sol_dist;
        int cnt[LIVE_MAX_W];             // detections by ring slot
        int has_marginal = 0;
        int64_t marginal_dropped = 0;
        double unc_sigma2 = 0;
        aar_tracker_detection_params det;
        MotionState ms;                  // the motion model: the member's two newest estimates, its last push's expected motion
        double last_rel[6];
        int last_predicted = 0;
    };
    aar_tracker_params prm;
    aar_lm_params lm;
    int B = 0, device = 0;
    hipStream_t stream = nullptr;
    std::vector<Member> mem;
    double *d_ent = nullptr, *d_K = nullptr;
    double *d_state = nullptr;           // [B][LIVE_ST_RES]: zslot | anchor | Ef | Pe of every member
    double *d_out = nullptr;             // [B][out_stride]: result | start record (| uncertainty record) of every member: ONE copy back
    char *d_ring = nullptr;              // [lag + 1][B] slots
    LiveMember *d_tab = nullptr;         // [B]
    char *h_stage = nullptr;             // pinned: [B] slots
    double *h_out = nullptr;             // pinned: [B][out_stride]
    size_t slot_bytes = 0, out_stride = 0, total_ent = 0, total_cams = 0;
    int64_t n = 0;
    double times[LIVE_MAX_W];
    bool unc_set = false;
    int unc_W = 0;
    bool det_on = false;
    void *d_cams = nullptr;
    double *d_toroot = nullptr, *d_work = nullptr;
    LiveInitMember *d_itab = nullptr;
    std::vector<int32_t> order;
    aar_tracker_bank_stats stats;
    // the gate (aar_tracker_gate_bank_enable); the members' gate records sit behind the [B][out_stride] block of d_out / h_out
    bool gate_on = false, gate_set = false;
    aar_tracker_gate_params gate;
    std::vector<double> gate_rec;        // [B][LIVE_GATE_DOUBLES] of the last accepted push
    LiveGateMember *d_gtab = nullptr;    // [B]
    double *d_gerr = nullptr;            // [B][max_obs_per_frame] e_d of the newest frames, then [B][max_obs_per_frame] keep flags (bytes)
    // the motion model (aar_tracker_motion_bank_enable): every ring slot then is the members' slots followed by their
    // expected motions [B][6]; the members' motion records sit behind the gate records of d_out / h_out
    bool motion_called = false, motion_on = false, motion_set = false;
    aar_tracker_motion_params motion;
    size_t ring_cap = 0, stage_cap = 0;  // bytes allocated
    size_t stride() const {              // of one ring slot of all members
        const size_t s = (size_t)B * slot_bytes;
        return motion_on ? (s + (size_t)B * 6 * sizeof(double) + 15) / 16 * 16 : s;
    }
};

namespace {

// an error of a member's check, with the member in front of the message
int bank_member_error(int rc, int b) {
    const std::string msg = aar_last_error();
    return set_error(rc, "member %d: %s", b, msg.c_str());
}

int bank_push(aar_tracker_bank *k, const char *fn, bool raw, double frame_time, const int32_t *n_obs, const int32_t *obs_cam, const int32_t *obs_marker,
              const float *obs_uv, const double *pose_init, const uint8_t *has_init, aar_tracker_result *results, aar_tracker_start_info *infos) {
    if (!k || !n_obs) return set_error(AAR_ERR_INVALID, "%s: null argument", fn);
    const auto t0 = std::chrono::steady_clock::now();
    const aar_tracker_params &p = k->prm;
    const int B = k->B, slots = p.lag + 1;
    const int64_t n = k->n;
    if (raw && !k->det_on) return set_error(AAR_ERR_INVALID, "%s: call aar_tracker_bank_enable_detections first", fn);
    // every member's input is checked before anything is touched: a bank push is all or nothing
    char who[32];
    size_t off = 0;
    for (int b = 0; b < B; b++) {
        snprintf(who, sizeof who, "member %d: ", b);
        const aar_tracker_bank::Member &m = k->mem[b];
        if (int rc = live_check_frame(fn, who, raw, m.C, m.M, p.max_obs_per_frame, n_obs[b], obs_cam ? obs_cam + off : nullptr,
                                      obs_marker ? obs_marker + off : nullptr, obs_uv ? obs_uv + 8 * off : nullptr))
            return rc;
        off += (size_t)n_obs[b];
    }
    if (!std::isfinite(frame_time)) return set_error(AAR_ERR_INVALID, "%s: frame_time is not finite", fn);
    const int ns = (int)(n % slots), ps = (int)((n + slots - 1) % slots);
    if (n > 0 && (!(frame_time > k->times[ps]) || !std::isfinite(frame_time - k->times[ps])))
        return set_error(AAR_ERR_INVALID, "%s: frame_time = %g does not ascend from the previous push's %g", fn, frame_time, k->times[ps]);
    bool all_init = true;
    for (int b = 0; b < B; b++) {
        snprintf(who, sizeof who, "member %d: ", b);
        const aar_tracker_bank::Member &m = k->mem[b];
        const double *init = pose_init && (!has_init || has_init[b]) ? pose_init + 6 * (size_t)b : nullptr;
        all_init = all_init && init;
        if (n == 0 && !init && !raw) return set_error(AAR_ERR_INVALID, "%s: %sthe first push needs a pose_init", fn, who);
        if (n == 0 && !init && !live_do_vote(m.det, n_obs[b], false))
            return set_error(AAR_ERR_INVALID, "%s: %sthe first push has %d detections, fewer than min_detections = %d, and no pose_init: nothing to start from",
                             fn, who, (int)n_obs[b], (int)m.det.min_detections);
        if (int rc = live_check_pose_init(fn, who, init)) return rc;
    }
    HIP_TRY(hipSetDevice(k->device));
    // the new slot of every member, staged one behind the other: ONE copy.  The header's idle doubles carry what differs by member.  With the
    // motion model the members' expected motions follow the slots in the same copy, and a member without a pose_init finds its prediction in the
    // header, where a pose_init would be
    const bool motion = k->motion_on;
    double *h_rel = reinterpret_cast<double *>(k->h_stage + (size_t)B * k->slot_bytes);   // [B][6] (motion only)
    std::vector<uint8_t> start_pred((size_t)B, 0), predicted((size_t)B, 0);
    size_t copy_bytes = 0;
    off = 0;
    for (int b = 0; b < B; b++) {
        char *slot = k->h_stage + (size_t)b * k->slot_bytes;
        const double *init = pose_init && (!has_init || has_init[b]) ? pose_init + 6 * (size_t)b : nullptr;
        const size_t used = live_stage_slot(slot, k->mem[b].C, raw, n_obs[b], obs_cam ? obs_cam + off : nullptr, obs_marker ? obs_marker + off : nullptr,
                                            obs_uv ? obs_uv + 8 * off : nullptr, init, k->order);
        double *hdr = reinterpret_cast<double *>(slot);
        hdr[LIVE_HDR_CNT] = (double)n_obs[b];
        hdr[LIVE_HDR_INIT] = init ? 1.0 : 0.0;
        if (motion) {
            double pred[6];
            predicted[b] = motion_measure(k->mem[b].ms, frame_time, k->motion.max_dt, h_rel + 6 * (size_t)b, pred) ? 1 : 0;
            if (!init && n > 0) {
                memcpy(hdr, pred, sizeof pred);
                if (!raw) hdr[LIVE_HDR_INIT] = 1.0;   // (raw: the start kernel takes it as its previous estimate, a vote is still held)
                start_pred[b] = 1;
            }
        }
        copy_bytes = (size_t)b * k->slot_bytes + used;
        off += (size_t)n_obs[b];
    }
    if (motion) copy_bytes = (size_t)B * k->slot_bytes + (size_t)B * 6 * sizeof(double);
    LiveBankArgs ba;
    memset(&ba, 0, sizeof ba);
    live_window_args(ba.sh, p, k->lm, n, frame_time, k->times);
    ba.sh.slot_bytes = k->stride();
    ba.tab = k->d_tab; ba.raw = raw ? 1 : 0; ba.fresh = n == 0 ? 1 : 0;
    const int W = ba.sh.W;
    const bool marginal = ba.sh.marginal != 0, tail = marginal || p.covariance;
    char *new_slots = k->d_ring + (size_t)ns * k->stride();
    aar_tracker_bank_stats &st = k->stats;
    HIP_TRY(hipMemcpyAsync(new_slots, k->h_stage, copy_bytes, hipMemcpyHostToDevice, k->stream));
    st.h2d_copies++; st.h2d_bytes += (int64_t)copy_bytes;
    const size_t out_bytes = (size_t)B * k->out_stride * sizeof(double);
    if (raw) {
        LiveInitBankArgs li;
        li.tab = k->d_itab; li.slot0 = new_slots; li.slot_bytes = k->slot_bytes; li.max_obs = (size_t)p.max_obs_per_frame;
        li.has_prev = n > 0 ? 1 : 0; li.prev_slot = ps; li.huber = ba.sh.huber;
        li.pred_in_header = motion ? 1 : 0;
        launch_live_init_bank(li, B, k->stream);
        st.launches++;
        if (n == 0 && !all_init) {
            // the only push a vote can fail with nothing to fall back on: read the start records before any window is touched
            HIP_TRY(hipMemcpyAsync(k->h_out, k->d_out, out_bytes, hipMemcpyDeviceToHost, k->stream));
            st.d2h_copies++; st.d2h_bytes += (int64_t)out_bytes;
            HIP_TRY(hipStreamSynchronize(k->stream));
            if (int rc = check_async("k_live_init_bank")) return rc;
            for (int b = 0; b < B; b++) {
                const double *h_info = k->h_out + (size_t)b * k->out_stride + LIVE_RES_DOUBLES;
                if (h_info[4] < 0.0)
                    return set_error(AAR_ERR_NUMERIC, "%s: member %d: no finite object pose candidate among %d, and neither a pose_init nor a previous estimate",
                                     fn, b, (int)h_info[1]);
            }
        }
    }
    const bool gate = k->gate_on;
    if (gate) {
        // every member's new slot compacted in place, the kept counts into the headers the refinement reads
        LiveGateBankArgs ga;
        ga.tab = k->d_gtab; ga.slot0 = new_slots; ga.slot_bytes = k->slot_bytes; ga.raw = raw ? 1 : 0; ga.prev_slot = ps;
        ga.g.k_median = k->gate.k_median; ga.g.min_px = k->gate.min_px; ga.g.min_detections = k->gate.min_detections;
        launch_live_gate_bank(ga, B, k->stream);
        st.launches++;
    }
    if (motion) {
        LiveBankMotionArgs bm;
        bm.ba = ba; bm.ring = k->d_ring; bm.rel_off = (size_t)B * k->slot_bytes;
        bm.mot = k->d_out + (size_t)B * k->out_stride + (size_t)B * LIVE_GATE_DOUBLES;   // [B][LIVE_MOT_DOUBLES], behind the gate records
        launch_live_push_bank_motion(bm, B, k->stream);
    } else {
        launch_live_push_bank(ba, B, k->stream);
    }
    st.launches++;
    if (tail) k->unc_set = false;   // the copy overwrites the records aar_tracker_bank_uncertainty serves
    const size_t back_bytes = out_bytes + (gate || motion ? (size_t)B * LIVE_GATE_DOUBLES * sizeof(double) : 0) +   // (the gate records ride behind: one copy)
                              (motion ? (size_t)B * LIVE_MOT_DOUBLES * sizeof(double) : 0);                            // (and behind them the motion records)
    HIP_TRY(hipMemcpyAsync(k->h_out, k->d_out, back_bytes, hipMemcpyDeviceToHost, k->stream));
    st.d2h_copies++; st.d2h_bytes += (int64_t)back_bytes;
    HIP_TRY(hipStreamSynchronize(k->stream));
    if (int rc = check_async("k_live_push_bank")) return rc;
    // the push is accepted
    for (int b = 0; b < B; b++) {
        aar_tracker_bank::Member &m = k->mem[b];
        const double *h = k->h_out + (size_t)b * k->out_stride;
        int kept = n_obs[b];
        if (gate) {   // later pushes, the rows and sigma2 see the compacted frame
            memcpy(&k->gate_rec[(size_t)b * LIVE_GATE_DOUBLES], k->h_out + (size_t)B * k->out_stride + (size_t)b * LIVE_GATE_DOUBLES,
                   LIVE_GATE_DOUBLES * sizeof(double));
            kept = (int)k->gate_rec[(size_t)b * LIVE_GATE_DOUBLES + 2];
        }
        if (tail) {
            // rows as the member's workgroup counted them (its has_marginal was the one this member held)
            int64_t det = kept;
            for (int i = 0; i < W - 1; i++) det += m.cnt[(ba.sh.first_slot + i) % slots];
            const double rows = live_rows(ba.sh, det, marginal ? m.has_marginal : 0);
            const double *u = h + LIVE_RES_DOUBLES + LIVE_INFO_DOUBLES;
            m.has_marginal = marginal && u[LIVE_UNC_HAS] != 0.0 ? 1 : 0;
            if (marginal && u[LIVE_UNC_DROP] != 0.0) m.marginal_dropped++;
            m.unc_sigma2 = live_sigma2(rows, W, h[4]);
        }
        m.cnt[ns] = kept;
        if (motion) {
            // the member's two newest estimates at this push's final point: its motion record and its result's newest pose
            MotionState &ms = m.ms;
            if (n > 0) { memcpy(ms.za, k->h_out + (size_t)B * k->out_stride + (size_t)B * LIVE_GATE_DOUBLES + (size_t)b * LIVE_MOT_DOUBLES, sizeof ms.za); ms.ta = ms.tb; }
            memcpy(ms.zb, h + 8, sizeof ms.zb);
            ms.tb = frame_time;
            ms.frames = n > 0 ? 2 : 1;
            memcpy(m.last_rel, h_rel + 6 * (size_t)b, sizeof m.last_rel);
            m.last_predicted = predicted[b];
            double *h_info = k->h_out + (size_t)b * k->out_stride + LIVE_RES_DOUBLES;
            if (raw && start_pred[b] && predicted[b] && h_info[4] == 1.0) h_info[4] = 3.0;   // the "previous estimate" was the motion prediction
        }
        if (results) live_fill_result(h, n, W, slots, t0, results + b);
        if (infos) live_fill_info(h + LIVE_RES_DOUBLES, infos + b);
    }
    if (motion) k->motion_set = true;
    if (tail) { k->unc_set = true; k->unc_W = W; }
    if (gate) k->gate_set = true;
    k->times[ns] = frame_time;
    k->n = n + 1;
    st.pushes++;
    return AAR_OK;
}

}  // namespace

int aar_tracker_bank_params_validate(int32_t n_members, const aar_dataset *const *solutions, const aar_tracker_params *in) {
    if (!solutions || !in) return set_error(AAR_ERR_INVALID, "aar_tracker_bank_params_validate: null argument");
    if (n_members < 1 || n_members > AAR_TRACKER_BANK_MAX_MEMBERS)
        return set_error(AAR_ERR_INVALID, "aar_tracker_bank: n_members = %d is outside 1 .. %d", (int)n_members, AAR_TRACKER_BANK_MAX_MEMBERS);
    for (int b = 0; b < n_members; b++) {
        if (!solutions[b]) return set_error(AAR_ERR_INVALID, "aar_tracker_bank: member %d: null solution", b);
        if (int rc = aar_tracker_params_validate(solutions[b], in)) return bank_member_error(rc, b);
    }
    return AAR_OK;
}

void aar_tracker_bank_destroy(aar_tracker_bank *k) {
    if (!k) return;
    (void)hipSetDevice(k->device);
    if (k->stream) (void)hipStreamSynchronize(k->stream);
    void *dev[] = {k->d_ent, k->d_K, k->d_state, k->d_out, k->d_ring, k->d_tab, k->d_cams, k->d_toroot, k->d_work, k->d_itab, k->d_gtab, k->d_gerr};
    for (void *q : dev)
        if (q) (void)hipFree(q);
    if (k->h_stage) (void)hipHostFree(k->h_stage);
    if (k->h_out) (void)hipHostFree(k->h_out);
    if (k->stream) (void)hipStreamDestroy(k->stream);
    delete k;
}

int aar_tracker_bank_create(int32_t n_members, const aar_dataset *const *solutions, const aar_tracker_params *in, const aar_lm_params *lm,
                            aar_tracker_bank **out) {
    if (!solutions || !in || !out) return set_error(AAR_ERR_INVALID, "aar_tracker_bank_create: null argument");
    *out = nullptr;
    int rc = aar_tracker_bank_params_validate(n_members, solutions, in);
    if (rc) return rc;
    aar_tracker_params p;
    (void)tracker_params_read(in, &p);
    if ((rc = ensure_device(p.device_id))) return rc;
    aar_tracker_bank *k = new aar_tracker_bank();
    const int B = n_members, slots = p.lag + 1;
    k->prm = p;
    if (lm) k->lm = *lm; else aar_lm_default_params(&k->lm);
    k->B = B; k->device = p.device_id;
    memset(&k->stats, 0, sizeof k->stats);
    k->stats.members = B;
    for (int i = 0; i < LIVE_MAX_W; i++) k->times[i] = 0.0;
    k->mem.resize((size_t)B);
    std::vector<double> z, Ks;
    for (int b = 0; b < B; b++) {
        const aar_dataset *sol = solutions[b];
        aar_tracker_bank::Member &m = k->mem[b];
        m.C = sol->num_cams; m.M = sol->num_markers; m.rc = sol->root_cam; m.rm = sol->root_marker;
        m.marker_size = sol->marker_size; m.half_size = (double)((float)sol->marker_size / 2.f);
        m.ent0 = k->total_ent; m.cam0 = k->total_cams;
        k->total_ent += (size_t)(m.C + m.M); k->total_cams += (size_t)m.C;
        if (sol->x_full) m.sol_x.assign(sol->x_full, sol->x_full + 6 * (size_t)(m.C - 1 + m.M - 1));
        m.sol_K.assign(sol->cam_mats, sol->cam_mats + 9 * (size_t)m.C);
        m.sol_dist.assign(5 * (size_t)m.C, 0.0);
        if (sol->dist_coeffs) m.sol_dist.assign(sol->dist_coeffs, sol->dist_coeffs + 5 * (size_t)m.C);
        for (int i = 0; i < LIVE_MAX_W; i++) m.cnt[i] = 0;
        aar_tracker_default_detection_params(&m.det);
        live_solution_z(sol, z);
        Ks.insert(Ks.end(), sol->cam_mats, sol->cam_mats + 9 * (size_t)m.C);
    }
    const bool tail = p.anchor_mode == AAR_TRACKER_ANCHOR_MARGINAL || p.covariance;
    k->slot_bytes = live_slot_bytes(p.max_obs_per_frame);
    k->out_stride = LIVE_RES_DOUBLES + LIVE_INFO_DOUBLES + (tail ? LIVE_UNC_HDR + (p.covariance ? 36 * (size_t)slots : 0) : 0);
    const size_t ring_bytes = (size_t)slots * B * k->slot_bytes, state_bytes = (size_t)B * LIVE_ST_RES * sizeof(double),
                 out_bytes = ((size_t)B * k->out_stride + (size_t)B * LIVE_GATE_DOUBLES + (size_t)B * LIVE_MOT_DOUBLES) * sizeof(double);   // (behind the records: the gate's, the motion model's)
    double *d_z = nullptr;
    auto fail = [&](int code) { if (d_z) (void)hipFree(d_z); aar_tracker_bank_destroy(k); return code; };
    if (hipStreamCreateWithFlags(&k->stream, hipStreamNonBlocking) != hipSuccess) return fail(set_error(AAR_ERR_HIP, "hipStreamCreate failed"));
    if (hipMalloc((void **)&k->d_ent, k->total_ent * ENT_STRIDE * sizeof(double)) != hipSuccess ||
        hipMalloc((void **)&k->d_K, 9 * k->total_cams * sizeof(double)) != hipSuccess || hipMalloc((void **)&k->d_state, state_bytes) != hipSuccess ||
        hipMalloc((void **)&k->d_out, out_bytes) != hipSuccess || hipMalloc((void **)&k->d_ring, ring_bytes) != hipSuccess ||
        hipMalloc((void **)&k->d_tab, (size_t)B * sizeof(LiveMember)) != hipSuccess || hipMalloc((void **)&d_z, z.size() * sizeof(double)) != hipSuccess)
        return fail(set_error(AAR_ERR_HIP, "aar_tracker_bank_create: hipMalloc failed (%d members, ring of %zu bytes)", B, ring_bytes));
    if (hipHostMalloc((void **)&k->h_stage, (size_t)B * k->slot_bytes, hipHostMallocDefault) != hipSuccess ||
        hipHostMalloc((void **)&k->h_out, out_bytes, hipHostMallocDefault) != hipSuccess)
        return fail(set_error(AAR_ERR_HIP, "aar_tracker_bank_create: hipHostMalloc failed"));
    memset(k->h_stage, 0, (size_t)B * k->slot_bytes);
    k->ring_cap = ring_bytes; k->stage_cap = (size_t)B * k->slot_bytes;
    if (hipMemsetAsync(k->d_state, 0, state_bytes, k->stream) != hipSuccess || hipMemsetAsync(k->d_out, 0, out_bytes, k->stream) != hipSuccess ||
        hipMemsetAsync(k->d_ring, 0, ring_bytes, k->stream) != hipSuccess)
        return fail(set_error(AAR_ERR_HIP, "aar_tracker_bank_create: hipMemset failed"));
    // the member table: written once
    std::vector<LiveMember> tab((size_t)B);
    for (int b = 0; b < B; b++) {
        const aar_tracker_bank::Member &m = k->mem[b];
        LiveMember &r = tab[b];
        double *stt = k->d_state + (size_t)b * LIVE_ST_RES;
        r.ent = k->d_ent + m.ent0 * ENT_STRIDE; r.Kmat = k->d_K + 9 * m.cam0; r.h = m.half_size;
        r.ring = k->d_ring + (size_t)b * k->slot_bytes;
        r.zslot = stt; r.anchor = stt + LIVE_ST_ANCHOR; r.Ef = stt + LIVE_ST_EF; r.Pe = stt + LIVE_ST_PE;
        r.res = k->d_out + (size_t)b * k->out_stride;
        r.unc = tail ? r.res + LIVE_RES_DOUBLES + LIVE_INFO_DOUBLES : nullptr;
    }
    const char *what = "";
    if (h2d(d_z, z.data(), z.size() * sizeof(double), k->stream, &what) || h2d(k->d_K, Ks.data(), Ks.size() * sizeof(double), k->stream, &what) ||
        h2d(k->d_tab, tab.data(), tab.size() * sizeof(LiveMember), k->stream, &what))
        return fail(set_error(AAR_ERR_HIP, "aar_tracker_bank_create: %s failed", what));
    // the entity rows of every member's fixed cameras and markers in ONE launch of the problem's unpack kernel (roots: the identity)
    DeviceProblem P;
    P.C = (int)k->total_ent; P.M = 0; P.A = (int)k->total_ent; P.F = 0; P.intr = 0;
    P.z[0] = d_z; P.ent[0] = k->d_ent;
    launch_unpack(P, 0, k->stream);
    if (hipStreamSynchronize(k->stream) != hipSuccess) return fail(set_error(AAR_ERR_HIP, "aar_tracker_bank_create: the unpack launch failed"));
    (void)hipFree(d_z);
    d_z = nullptr;
    if ((rc = check_async("tracker bank creation"))) return fail(rc);
    *out = k;
    return AAR_OK;
}

int32_t aar_tracker_bank_size(const aar_tracker_bank *k) { return k ? k->B : 0; }

int aar_tracker_bank_reset(aar_tracker_bank *k) {
    if (!k) return set_error(AAR_ERR_INVALID, "aar_tracker_bank_reset: null argument");
    k->n = 0;
    k->det_on = false;   // (the buffers stay; aar_tracker_bank_enable_detections fills them again)
    k->gate_on = false;  // (likewise aar_tracker_gate_bank_enable)
    k->gate_set = false;
    k->motion_called = k->motion_on = k->motion_set = false;   // (likewise aar_tracker_motion_bank_enable; the larger ring stays allocated)
    k->unc_set = false;  // (the device's marginals stay where they are: the first push of a bank reads none)
    for (auto &m : k->mem) { m.has_marginal = 0; m.marginal_dropped = 0; m.ms = MotionState(); }
    return AAR_OK;
}

int aar_tracker_bank_push(aar_tracker_bank *k, double frame_time, const int32_t *n_obs, const int32_t *obs_cam, const int32_t *obs_marker,
                          const float *obs_uv, const double *pose_init, const uint8_t *has_init, aar_tracker_result *results) {
    return bank_push(k, "aar_tracker_bank_push", false, frame_time, n_obs, obs_cam, obs_marker, obs_uv, pose_init, has_init, results, nullptr);
}

int aar_tracker_bank_push_detections(aar_tracker_bank *k, double frame_time, const int32_t *n_det, const int32_t *det_cam, const int32_t *det_marker,
                                     const float *det_uv_raw, const double *pose_init, const uint8_t *has_init, aar_tracker_result *results,
                                     aar_tracker_start_info *infos) {
    return bank_push(k, "aar_tracker_bank_push_detections", true, frame_time, n_det, det_cam, det_marker, det_uv_raw, pose_init, has_init, results, infos);
}

int aar_tracker_bank_enable_detections(aar_tracker_bank *k, const aar_tracker_detection_params *const *per_member) {
    if (!k) {   // no bank exists without a device: say which of the two it is
        if (int rc = ensure_device(0)) return rc;
        return set_error(AAR_ERR_INVALID, "aar_tracker_bank_enable_detections: null bank");
    }
    if (k->det_on) return set_error(AAR_ERR_INVALID, "aar_tracker_bank_enable_detections: already enabled (aar_tracker_bank_reset first)");
    if (k->n != 0)
        return set_error(AAR_ERR_INVALID, "aar_tracker_bank_enable_detections: call it after aar_tracker_bank_create or aar_tracker_bank_reset, before the first push");
    const int B = k->B;
    aar_tracker_detection_params dflt;
    aar_tracker_default_detection_params(&dflt);
    std::vector<aar_tracker_detection_params> det((size_t)B);
    for (int b = 0; b < B; b++)
        if (int rc = detection_params_check(k->mem[b].C, per_member && per_member[b] ? per_member[b] : &dflt, &det[b])) return bank_member_error(rc, b);
    if (k->prm.max_obs_per_frame > LIVE_DET_MAX_OBS)
        return set_error(AAR_ERR_UNSUPPORTED, "aar_tracker_bank_enable_detections: max_obs_per_frame = %d is above %d (a member's vote runs in one workgroup)",
                         (int)k->prm.max_obs_per_frame, LIVE_DET_MAX_OBS);
    HIP_TRY(hipSetDevice(k->device));
    const size_t mo = (size_t)k->prm.max_obs_per_frame, work = live_init_work_doubles(mo), cam_row = 9 + AAR_MAX_DIST;
    if (!k->d_cams) HIP_TRY(hipMalloc(&k->d_cams, k->total_cams * cam_row * sizeof(double)));
    if (!k->d_toroot) HIP_TRY(hipMalloc((void **)&k->d_toroot, 12 * k->total_ent * sizeof(double)));
    if (!k->d_work) HIP_TRY(hipMalloc((void **)&k->d_work, (size_t)B * work * sizeof(double)));
    if (!k->d_itab) HIP_TRY(hipMalloc((void **)&k->d_itab, (size_t)B * sizeof(LiveInitMember)));
    std::vector<double> tab(k->total_cams * cam_row, 0.0), tr(12 * k->total_ent, 0.0);
    std::vector<LiveInitMember> itab((size_t)B);
    for (int b = 0; b < B; b++) {
        const aar_tracker_bank::Member &m = k->mem[b];
        live_detection_tables(m.C, m.M, m.rc, m.rm, det[b].cams, m.sol_x.data(), m.sol_K.data(), m.sol_dist.data(), &tab[m.cam0 * cam_row], &tr[12 * m.ent0]);
        LiveInitMember &r = itab[b];
        r.cams = reinterpret_cast<const double *>(k->d_cams) + m.cam0 * cam_row;
        r.Tcr = k->d_toroot + 12 * m.ent0; r.Tmr = r.Tcr + 12 * (size_t)m.C;
        r.C = m.C; r.policy = det[b].start_policy; r.min_detections = det[b].min_detections;
        r.hf = (float)m.marker_size / 2.0f; r.h = m.marker_size / 2; r.threshold = det[b].ippe_threshold;   // as the Initializer: float for IPPE, double for the vote
        r.ent = k->d_ent + m.ent0 * ENT_STRIDE; r.Kmat = k->d_K + 9 * m.cam0; r.h_track = m.half_size;
        r.zslot = k->d_state + (size_t)b * LIVE_ST_RES;
        r.work = k->d_work + (size_t)b * work;
        r.info = k->d_out + (size_t)b * k->out_stride + LIVE_RES_DOUBLES;
    }
    const char *what = "";
    if (h2d(k->d_cams, tab.data(), tab.size() * sizeof(double), k->stream, &what) || h2d(k->d_toroot, tr.data(), tr.size() * sizeof(double), k->stream, &what) ||
        h2d(k->d_itab, itab.data(), itab.size() * sizeof(LiveInitMember), k->stream, &what))
        return set_error(AAR_ERR_HIP, "aar_tracker_bank_enable_detections: %s failed", what);
    HIP_TRY(hipStreamSynchronize(k->stream));
    for (int b = 0; b < B; b++) {
        det[b].cams = nullptr;   // (copied; the caller's array is not kept)
        k->mem[b].det = det[b];
    }
    k->det_on = true;
    return AAR_OK;
}

int aar_tracker_bank_uncertainty(aar_tracker_bank *k, int32_t member, aar_tracker_uncertainty_record *out) {
    if (!k || !out) return set_error(AAR_ERR_INVALID, "aar_tracker_bank_uncertainty: null argument");
    if (member < 0 || member >= k->B) return set_error(AAR_ERR_INVALID, "aar_tracker_bank_uncertainty: member = %d is outside 0 .. %d", (int)member, k->B - 1);
    if (k->prm.anchor_mode == AAR_TRACKER_ANCHOR_FIXED && !k->prm.covariance)
        return set_error(AAR_ERR_INVALID, "aar_tracker_bank_uncertainty: the bank was created with anchor_mode fixed and covariance = 0: nothing is kept");
    if (!k->unc_set || k->n == 0) return set_error(AAR_ERR_INVALID, "aar_tracker_bank_uncertainty: no push since creation / reset");
    if (out->struct_size < offsetof(aar_tracker_uncertainty_record, cov_valid) + sizeof(int32_t))
        return set_error(AAR_ERR_INVALID, "aar_tracker_bank_uncertainty: struct_size %u does not reach cov_valid", (unsigned)out->struct_size);
    const aar_tracker_bank::Member &m = k->mem[member];
    live_fill_uncertainty(k->prm, k->h_out + (size_t)member * k->out_stride + LIVE_RES_DOUBLES + LIVE_INFO_DOUBLES, k->unc_W, k->n, m.has_marginal,
                          m.marginal_dropped, m.unc_sigma2, out);
    return AAR_OK;
}

int aar_tracker_bank_window(aar_tracker_bank *k, int32_t member, int32_t *n_out, int64_t *frame_index, double *poses, double *frame_err, double *pair_err,
                            double anchor_pose[6], int32_t *has_anchor) {
    if (!k) return set_error(AAR_ERR_INVALID, "aar_tracker_bank_window: null argument");
    if (member < 0 || member >= k->B) return set_error(AAR_ERR_INVALID, "aar_tracker_bank_window: member = %d is outside 0 .. %d", (int)member, k->B - 1);
    const int slots = k->prm.lag + 1;
    live_window_out(nullptr, k->n, slots, n_out, frame_index, poses, frame_err, pair_err, anchor_pose, has_anchor);
    if (k->n == 0 || (!poses && !frame_err && !pair_err && !anchor_pose)) return AAR_OK;
    HIP_TRY(hipSetDevice(k->device));
    double st[LIVE_ST_RES];
    const char *what = "";
    if (d2h(st, k->d_state + (size_t)member * LIVE_ST_RES, sizeof st, k->stream, &what)) return set_error(AAR_ERR_HIP, "aar_tracker_bank_window: %s failed", what);
    live_window_out(st, k->n, slots, nullptr, nullptr, poses, frame_err, pair_err, anchor_pose, nullptr);
    return AAR_OK;
}

int aar_tracker_bank_get_stats(const aar_tracker_bank *k, aar_tracker_bank_stats *out) {
    if (!k || !out) return set_error(AAR_ERR_INVALID, "aar_tracker_bank_get_stats: null argument");
    const size_t cap = out->struct_size;
    if (cap < 2 * sizeof(int32_t) || cap > 4096)
        return set_error(AAR_ERR_INVALID, "aar_tracker_bank_stats.struct_size is not set (sizeof(aar_tracker_bank_stats) of the caller)");
    aar_tracker_bank_stats st = k->stats;
    st.struct_size = (uint32_t)std::min(cap, sizeof st);
    memcpy(out, &st, std::min(cap, sizeof st));
    return AAR_OK;
}

// ------------------------------------------------------------------------------------------------
// The gate of the live trackers (live_gate_kernels.hip)
// ------------------------------------------------------------------------------------------------
namespace {

// the tracker as the one member of a bank (the gated refinement): the same state, the records where the single tracker's kernels leave them --
// behind the motion record in the model's own block when the motion model is on
int tracker_write_member_row(aar_tracker *t, const char *fn) {
    LiveMember r;
    r.ent = t->d_ent; r.Kmat = t->d_K; r.h = t->half_size; r.ring = t->d_ring;
    r.zslot = t->d_state; r.anchor = t->d_state + LIVE_ST_ANCHOR; r.Ef = t->d_state + LIVE_ST_EF; r.Pe = t->d_state + LIVE_ST_PE;
    r.res = t->motion_on ? t->d_mot + LIVE_MOT_DOUBLES + LIVE_GATE_DOUBLES : t->d_state + LIVE_ST_RES;
    r.unc = r.res + LIVE_RES_DOUBLES + LIVE_INFO_DOUBLES;
    const char *what = "";
    if (h2d(t->d_gtab, &r, sizeof r, t->stream, &what)) return set_error(AAR_ERR_HIP, "%s: %s failed", fn, what);
    HIP_TRY(hipStreamSynchronize(t->stream));
    return AAR_OK;
}

int gate_params_check(const aar_tracker_gate_params *in, aar_tracker_gate_params *p) {
    aar_tracker_default_gate_params(p);
    if (in->struct_size < offsetof(aar_tracker_gate_params, min_detections) + sizeof(int32_t))
        return set_error(AAR_ERR_INVALID, "aar_tracker_gate_params: struct_size %u does not reach min_detections", (unsigned)in->struct_size);
    memcpy(p, in, std::min<size_t>(in->struct_size, sizeof *p));
    p->struct_size = (uint32_t)sizeof *p;
    if (!std::isfinite(p->min_px) || p->min_px < 0.0) return set_error(AAR_ERR_INVALID, "aar_tracker_gate_params: min_px = %g must be finite and not negative", p->min_px);
    if (!std::isfinite(p->k_median)) return set_error(AAR_ERR_INVALID, "aar_tracker_gate_params: k_median = %g must be finite", p->k_median);
    if (p->k_median <= 0.0 && p->min_px <= 0.0)
        return set_error(AAR_ERR_INVALID, "aar_tracker_gate_params: k_median = %g and min_px = %g are both <= 0: no threshold", p->k_median, p->min_px);
    if (p->min_detections < 1) return set_error(AAR_ERR_INVALID, "aar_tracker_gate_params: min_detections = %d must be at least 1", (int)p->min_detections);
    return AAR_OK;
}

int gate_fill_info(const char *fn, const double *rec, aar_tracker_gate_info *out) {
    if (out->struct_size < offsetof(aar_tracker_gate_info, gated) + sizeof(int32_t))
        return set_error(AAR_ERR_INVALID, "%s: struct_size %u does not reach gated", fn, (unsigned)out->struct_size);
    aar_tracker_gate_info r;
    memset(&r, 0, sizeof r);
    r.struct_size = (uint32_t)std::min<size_t>(out->struct_size, sizeof r);
    r.gated = (int32_t)rec[0]; r.n_in = (int32_t)rec[1]; r.n_kept = (int32_t)rec[2]; r.n_nonfinite = (int32_t)rec[3];
    r.median = rec[4]; r.max = rec[5]; r.threshold = rec[6];
    memcpy(out, &r, r.struct_size);
    return AAR_OK;
}

// e_d and the keep flags of a newest frame of n detections: the second copy, made only here
int gate_detail_out(const char *fn, hipStream_t stream, const double *d_err, const uint8_t *d_keep, int n, int32_t *n_out, double *det_err, uint8_t *keep) {
    if (n_out) *n_out = n;
    const char *what = "";
    if (n > 0 && det_err && d2h(det_err, d_err, (size_t)n * sizeof(double), stream, &what)) return set_error(AAR_ERR_HIP, "%s: %s failed", fn, what);
    if (n > 0 && keep && d2h(keep, d_keep, (size_t)n, stream, &what)) return set_error(AAR_ERR_HIP, "%s: %s failed", fn, what);
    return AAR_OK;
}

}  // namespace

void aar_tracker_default_gate_params(aar_tracker_gate_params *p) {
    if (!p) return;
    memset(p, 0, sizeof *p);
    p->struct_size = (uint32_t)sizeof *p;
    p->k_median = 6.0;
    p->min_px = 3.0;
    p->min_detections = 4;
}

int aar_tracker_gate_params_validate(const aar_tracker_gate_params *in) {
    if (!in) return set_error(AAR_ERR_INVALID, "aar_tracker_gate_params_validate: null argument");
    aar_tracker_gate_params p;
    return gate_params_check(in, &p);
}

int aar_tracker_enable_gate(aar_tracker *t, const aar_tracker_gate_params *in) {
    if (!in) return set_error(AAR_ERR_INVALID, "aar_tracker_enable_gate: null argument");
    aar_tracker_gate_params p;
    if (int rc = gate_params_check(in, &p)) return rc;
    if (!t) {   // no tracker exists without a device: say which of the two it is
        if (int rc = ensure_device(0)) return rc;
        return set_error(AAR_ERR_INVALID, "aar_tracker_enable_gate: null tracker");
    }
    if (t->gate_on) return set_error(AAR_ERR_INVALID, "aar_tracker_enable_gate: already enabled (aar_tracker_reset first)");
    if (t->n != 0) return set_error(AAR_ERR_INVALID, "aar_tracker_enable_gate: call it after aar_tracker_create or aar_tracker_reset, before the first push");
    if (t->prm.max_obs_per_frame > LIVE_GATE_MAX_OBS)
        return set_error(AAR_ERR_UNSUPPORTED, "aar_tracker_enable_gate: max_obs_per_frame = %d is above %d (the median sorts the frame in one workgroup)",
                         (int)t->prm.max_obs_per_frame, LIVE_GATE_MAX_OBS);
    HIP_TRY(hipSetDevice(t->device));
    const size_t mo = (size_t)t->prm.max_obs_per_frame;
    if (!t->d_gerr) HIP_TRY(hipMalloc((void **)&t->d_gerr, mo * sizeof(double) + mo));
    if (!t->d_gtab) HIP_TRY(hipMalloc((void **)&t->d_gtab, sizeof(LiveMember)));
    if (int rc = tracker_write_member_row(t, "aar_tracker_enable_gate")) return rc;
    t->gate = p;
    t->gate_on = true;
    t->gate_set = false;
    return AAR_OK;
}

int aar_tracker_last_gate(aar_tracker *t, aar_tracker_gate_info *out) {
    if (!t || !out) return set_error(AAR_ERR_INVALID, "aar_tracker_last_gate: null argument");
    if (!t->gate_on) return set_error(AAR_ERR_INVALID, "aar_tracker_last_gate: the tracker has no gate (aar_tracker_enable_gate)");
    if (!t->gate_set || t->n == 0) return set_error(AAR_ERR_INVALID, "aar_tracker_last_gate: no push since creation / reset");
    return gate_fill_info("aar_tracker_last_gate", t->gate_rec, out);
}

int aar_tracker_gate_detail(aar_tracker *t, int32_t *n, double *det_err, uint8_t *keep) {
    if (!t) return set_error(AAR_ERR_INVALID, "aar_tracker_gate_detail: null argument");
    if (!t->gate_on) return set_error(AAR_ERR_INVALID, "aar_tracker_gate_detail: the tracker has no gate (aar_tracker_enable_gate)");
    if (!t->gate_set || t->n == 0) return set_error(AAR_ERR_INVALID, "aar_tracker_gate_detail: no push since creation / reset");
    HIP_TRY(hipSetDevice(t->device));
    return gate_detail_out("aar_tracker_gate_detail", t->stream, t->d_gerr, reinterpret_cast<const uint8_t *>(t->d_gerr + (size_t)t->prm.max_obs_per_frame),
                           (int)t->gate_rec[1], n, det_err, keep);
}

int aar_tracker_gate_bank_enable(aar_tracker_bank *k, const aar_tracker_gate_params *in) {
    if (!in) return set_error(AAR_ERR_INVALID, "aar_tracker_gate_bank_enable: null argument");
    aar_tracker_gate_params p;
    if (int rc = gate_params_check(in, &p)) return rc;
    if (!k) {   // no bank exists without a device: say which of the two it is
        if (int rc = ensure_device(0)) return rc;
        return set_error(AAR_ERR_INVALID, "aar_tracker_gate_bank_enable: null bank");
    }
    if (k->gate_on) return set_error(AAR_ERR_INVALID, "aar_tracker_gate_bank_enable: already enabled (aar_tracker_bank_reset first)");
    if (k->n != 0)
        return set_error(AAR_ERR_INVALID, "aar_tracker_gate_bank_enable: call it after aar_tracker_bank_create or aar_tracker_bank_reset, before the first push");
    if (k->prm.max_obs_per_frame > LIVE_GATE_MAX_OBS)
        return set_error(AAR_ERR_UNSUPPORTED, "aar_tracker_gate_bank_enable: max_obs_per_frame = %d is above %d (a member's median sorts its frame in one workgroup)",
                         (int)k->prm.max_obs_per_frame, LIVE_GATE_MAX_OBS);
    HIP_TRY(hipSetDevice(k->device));
    const int B = k->B;
    const size_t mo = (size_t)k->prm.max_obs_per_frame;
    if (!k->d_gerr) HIP_TRY(hipMalloc((void **)&k->d_gerr, (size_t)B * (mo * sizeof(double) + mo)));
    if (!k->d_gtab) {
        HIP_TRY(hipMalloc((void **)&k->d_gtab, (size_t)B * sizeof(LiveGateMember)));
        std::vector<LiveGateMember> tab((size_t)B);
        for (int b = 0; b < B; b++) {
            const aar_tracker_bank::Member &m = k->mem[b];
            LiveGateMember &r = tab[b];
            r.ent = k->d_ent + m.ent0 * ENT_STRIDE; r.Kmat = k->d_K + 9 * m.cam0; r.h = m.half_size;
            r.zslot = k->d_state + (size_t)b * LIVE_ST_RES;
            r.rec = k->d_out + (size_t)B * k->out_stride + (size_t)b * LIVE_GATE_DOUBLES;
            r.det_err = k->d_gerr + (size_t)b * mo;
            r.keep = reinterpret_cast<uint8_t *>(k->d_gerr + (size_t)B * mo) + (size_t)b * mo;
        }
        const char *what = "";
        if (h2d(k->d_gtab, tab.data(), tab.size() * sizeof(LiveGateMember), k->stream, &what))
            return set_error(AAR_ERR_HIP, "aar_tracker_gate_bank_enable: %s failed", what);
        HIP_TRY(hipStreamSynchronize(k->stream));
    }
    k->gate_rec.assign((size_t)B * LIVE_GATE_DOUBLES, 0.0);
    k->gate = p;
    k->gate_on = true;
    k->gate_set = false;
    return AAR_OK;
}

int aar_tracker_gate_bank_last(aar_tracker_bank *k, int32_t member, aar_tracker_gate_info *out) {
    if (!k || !out) return set_error(AAR_ERR_INVALID, "aar_tracker_gate_bank_last: null argument");
    if (member < 0 || member >= k->B) return set_error(AAR_ERR_INVALID, "aar_tracker_gate_bank_last: member = %d is outside 0 .. %d", (int)member, k->B - 1);
    if (!k->gate_on) return set_error(AAR_ERR_INVALID, "aar_tracker_gate_bank_last: the bank has no gate (aar_tracker_gate_bank_enable)");
    if (!k->gate_set || k->n == 0) return set_error(AAR_ERR_INVALID, "aar_tracker_gate_bank_last: no push since creation / reset");
    return gate_fill_info("aar_tracker_gate_bank_last", &k->gate_rec[(size_t)member * LIVE_GATE_DOUBLES], out);
}

int aar_tracker_gate_bank_detail(aar_tracker_bank *k, int32_t member, int32_t *n, double *det_err, uint8_t *keep) {
    if (!k) return set_error(AAR_ERR_INVALID, "aar_tracker_gate_bank_detail: null argument");
    if (member < 0 || member >= k->B) return set_error(AAR_ERR_INVALID, "aar_tracker_gate_bank_detail: member = %d is outside 0 .. %d", (int)member, k->B - 1);
    if (!k->gate_on) return set_error(AAR_ERR_INVALID, "aar_tracker_gate_bank_detail: the bank has no gate (aar_tracker_gate_bank_enable)");
    if (!k->gate_set || k->n == 0) return set_error(AAR_ERR_INVALID, "aar_tracker_gate_bank_detail: no push since creation / reset");
    HIP_TRY(hipSetDevice(k->device));
    const size_t mo = (size_t)k->prm.max_obs_per_frame;
    return gate_detail_out("aar_tracker_gate_bank_detail", k->stream, k->d_gerr + (size_t)member * mo,
                           reinterpret_cast<const uint8_t *>(k->d_gerr + (size_t)k->B * mo) + (size_t)member * mo,
                           (int)k->gate_rec[(size_t)member * LIVE_GATE_DOUBLES + 1], n, det_err, keep);
}

// ---- constant-velocity motion model of the live tracker ----
namespace {

// a tracker's block of push records with the model: motion record | gate record | result | start record | uncertainty record
constexpr size_t LIVE_MOT_BLOCK = LIVE_MOT_DOUBLES + LIVE_GATE_DOUBLES + LIVE_RES_DOUBLES + LIVE_INFO_DOUBLES + LIVE_UNC_DOUBLES;

int motion_params_check(const aar_tracker_params *tp, const aar_tracker_motion_params *in, aar_tracker_motion_params *p) {
    aar_tracker_default_motion_params(p);
    if (in->struct_size < offsetof(aar_tracker_motion_params, model) + sizeof(int32_t))
        return set_error(AAR_ERR_INVALID, "aar_tracker_motion_params: struct_size %u does not reach model", (unsigned)in->struct_size);
    memcpy(p, in, std::min<size_t>(in->struct_size, sizeof *p));
    p->struct_size = (uint32_t)sizeof *p;
    if (p->model != AAR_TRACKER_MOTION_RANDOM_WALK && p->model != AAR_TRACKER_MOTION_CONSTANT_VELOCITY)
        return set_error(AAR_ERR_INVALID, "aar_tracker_motion_params: model = %d is neither AAR_TRACKER_MOTION_RANDOM_WALK nor AAR_TRACKER_MOTION_CONSTANT_VELOCITY",
                         (int)p->model);
    if (!std::isfinite(p->max_dt) || p->max_dt < 0.0)
        return set_error(AAR_ERR_INVALID, "aar_tracker_motion_params: max_dt = %g must be finite and not negative", p->max_dt);
    aar_tracker_params q;
    if (!tracker_params_read(tp, &q))
        return set_error(AAR_ERR_INVALID, "aar_tracker_params: struct_size %u does not reach lag / smooth", (unsigned)tp->struct_size);
    if (p->model == AAR_TRACKER_MOTION_CONSTANT_VELOCITY && !q.smooth)
        return set_error(AAR_ERR_INVALID, "aar_tracker_motion_params: model = AAR_TRACKER_MOTION_CONSTANT_VELOCITY needs smooth = 1 (the prior carries the expected motion)");
    return AAR_OK;
}

}  // namespace

void aar_tracker_default_motion_params(aar_tracker_motion_params *p) {
    if (!p) return;
    memset(p, 0, sizeof *p);
    p->struct_size = (uint32_t)sizeof *p;
    p->model = AAR_TRACKER_MOTION_CONSTANT_VELOCITY;
    p->max_dt = 0.0;
}

int aar_tracker_motion_params_validate(const aar_tracker_params *tp, const aar_tracker_motion_params *in) {
    if (!tp || !in) return set_error(AAR_ERR_INVALID, "aar_tracker_motion_params_validate: null argument");
    aar_tracker_motion_params p;
    return motion_params_check(tp, in, &p);
}

int aar_tracker_enable_motion(aar_tracker *t, const aar_tracker_motion_params *in) {
    if (!in) return set_error(AAR_ERR_INVALID, "aar_tracker_enable_motion: null argument");
    if (!t) {   // no tracker exists without a device: say which of the two it is
        if (int rc = ensure_device(0)) return rc;
        return set_error(AAR_ERR_INVALID, "aar_tracker_enable_motion: null tracker");
    }
    aar_tracker_motion_params p;
    if (int rc = motion_params_check(&t->prm, in, &p)) return rc;
    if (t->motion_called) return set_error(AAR_ERR_INVALID, "aar_tracker_enable_motion: already called (aar_tracker_reset first)");
    if (t->n != 0) return set_error(AAR_ERR_INVALID, "aar_tracker_enable_motion: call it after aar_tracker_create or aar_tracker_reset, before the first push");
    if (p.model == AAR_TRACKER_MOTION_RANDOM_WALK) {   // the tracker stays as it is
        t->motion_called = true;
        return AAR_OK;
    }
    HIP_TRY(hipSetDevice(t->device));
    const size_t doubles = LIVE_MOT_BLOCK;
    if (!t->d_mot) HIP_TRY(hipMalloc((void **)&t->d_mot, doubles * sizeof(double)));
    if (!t->h_mot) HIP_TRY(hipHostMalloc((void **)&t->h_mot, doubles * sizeof(double), hipHostMallocDefault));
    HIP_TRY(hipMemsetAsync(t->d_mot, 0, doubles * sizeof(double), t->stream));
    HIP_TRY(hipStreamSynchronize(t->stream));
    memset(t->h_mot, 0, doubles * sizeof(double));
    t->h_res = t->h_mot + LIVE_MOT_DOUBLES + LIVE_GATE_DOUBLES;
    t->motion = p;
    t->mstate = MotionState();
    memset(t->rel_slot, 0, sizeof t->rel_slot);
    t->motion_called = t->motion_on = true;
    t->motion_set = false;
    if (t->gate_on) return tracker_write_member_row(t, "aar_tracker_enable_motion");   // the gated refinement's records move with the others
    return AAR_OK;
}

int aar_tracker_last_motion(aar_tracker *t, aar_tracker_motion_info *out) {
    if (!t || !out) return set_error(AAR_ERR_INVALID, "aar_tracker_last_motion: null argument");
    if (!t->motion_on) return set_error(AAR_ERR_INVALID, "aar_tracker_last_motion: the tracker has no motion model (aar_tracker_enable_motion)");
    if (!t->motion_set || t->n == 0) return set_error(AAR_ERR_INVALID, "aar_tracker_last_motion: no push since creation / reset");
    if (out->struct_size < offsetof(aar_tracker_motion_info, predicted) + sizeof(int32_t))
        return set_error(AAR_ERR_INVALID, "aar_tracker_last_motion: struct_size %u does not reach predicted", (unsigned)out->struct_size);
    aar_tracker_motion_info r;
    memset(&r, 0, sizeof r);
    r.struct_size = (uint32_t)std::min<size_t>(out->struct_size, sizeof r);
    r.model = t->motion.model; r.predicted = t->last_predicted;
    memcpy(r.rel, t->last_rel, sizeof r.rel);
    motion_velocity(t->mstate, r.velocity);
    r.newest_time = t->mstate.tb;
    memcpy(out, &r, r.struct_size);
    return AAR_OK;
}

int aar_tracker_predict(aar_tracker *t, double time, double pose[6]) {
    if (!t || !pose) return set_error(AAR_ERR_INVALID, "aar_tracker_predict: null argument");
    if (!t->motion_on) return set_error(AAR_ERR_INVALID, "aar_tracker_predict: the tracker has no motion model (aar_tracker_enable_motion)");
    if (!t->motion_set || t->n == 0) return set_error(AAR_ERR_INVALID, "aar_tracker_predict: no push since creation / reset");
    if (!std::isfinite(time) || time < t->mstate.tb)
        return set_error(AAR_ERR_INVALID, "aar_tracker_predict: time = %g is not finite or lies before the newest frame's %g", time, t->mstate.tb);
    motion_predict(t->mstate, time, t->motion.max_dt, pose);
    return AAR_OK;
}

int aar_tracker_motion_bank_enable(aar_tracker_bank *k, const aar_tracker_motion_params *in) {
    if (!in) return set_error(AAR_ERR_INVALID, "aar_tracker_motion_bank_enable: null argument");
    if (!k) {   // no bank exists without a device: say which of the two it is
        if (int rc = ensure_device(0)) return rc;
        return set_error(AAR_ERR_INVALID, "aar_tracker_motion_bank_enable: null bank");
    }
    aar_tracker_motion_params p;
    if (int rc = motion_params_check(&k->prm, in, &p)) return rc;
    if (k->motion_called) return set_error(AAR_ERR_INVALID, "aar_tracker_motion_bank_enable: already called (aar_tracker_bank_reset first)");
    if (k->n != 0)
        return set_error(AAR_ERR_INVALID, "aar_tracker_motion_bank_enable: call it after aar_tracker_bank_create or aar_tracker_bank_reset, before the first push");
    if (p.model == AAR_TRACKER_MOTION_RANDOM_WALK) {   // the bank stays as it is
        k->motion_called = true;
        return AAR_OK;
    }
    HIP_TRY(hipSetDevice(k->device));
    // room for the members' expected motions behind their slots, in the ring and in the staging buffer (the ring is empty: no frame is lost)
    const int B = k->B, slots = k->prm.lag + 1;
    k->motion_on = true;
    const size_t stride = k->stride();
    auto fail = [&](int code) { k->motion_on = false; return code; };
    if (k->ring_cap < (size_t)slots * stride || k->stage_cap < stride) {
        char *ring = nullptr, *stage = nullptr;
        if (hipMalloc((void **)&ring, (size_t)slots * stride) != hipSuccess || hipHostMalloc((void **)&stage, stride, hipHostMallocDefault) != hipSuccess) {
            if (ring) (void)hipFree(ring);
            return fail(set_error(AAR_ERR_HIP, "aar_tracker_motion_bank_enable: allocation failed (ring of %zu bytes)", (size_t)slots * stride));
        }
        (void)hipStreamSynchronize(k->stream);
        (void)hipFree(k->d_ring);
        (void)hipHostFree(k->h_stage);
        k->d_ring = ring; k->h_stage = stage;
        k->ring_cap = (size_t)slots * stride; k->stage_cap = stride;
        memset(k->h_stage, 0, stride);
        // the member table's ring pointers follow
        std::vector<LiveMember> tab((size_t)B);
        const char *what = "";
        if (d2h(tab.data(), k->d_tab, tab.size() * sizeof(LiveMember), k->stream, &what)) return fail(set_error(AAR_ERR_HIP, "aar_tracker_motion_bank_enable: %s failed", what));
        for (int b = 0; b < B; b++) tab[b].ring = k->d_ring + (size_t)b * k->slot_bytes;
        if (h2d(k->d_tab, tab.data(), tab.size() * sizeof(LiveMember), k->stream, &what)) return fail(set_error(AAR_ERR_HIP, "aar_tracker_motion_bank_enable: %s failed", what));
    }
    if (hipMemsetAsync(k->d_ring, 0, (size_t)slots * stride, k->stream) != hipSuccess || hipStreamSynchronize(k->stream) != hipSuccess)
        return fail(set_error(AAR_ERR_HIP, "aar_tracker_motion_bank_enable: hipMemset failed"));
    for (auto &m : k->mem) { m.ms = MotionState(); memset(m.last_rel, 0, sizeof m.last_rel); m.last_predicted = 0; }
    k->motion = p;
    k->motion_called = true;
    k->motion_set = false;
    return AAR_OK;
}

int aar_tracker_motion_bank_last(aar_tracker_bank *k, int32_t member, aar_tracker_motion_info *out) {
    if (!k || !out) return set_error(AAR_ERR_INVALID, "aar_tracker_motion_bank_last: null argument");
    if (member < 0 || member >= k->B) return set_error(AAR_ERR_INVALID, "aar_tracker_motion_bank_last: member = %d is outside 0 .. %d", (int)member, k->B - 1);
    if (!k->motion_on) return set_error(AAR_ERR_INVALID, "aar_tracker_motion_bank_last: the bank has no motion model (aar_tracker_motion_bank_enable)");
    if (!k->motion_set || k->n == 0) return set_error(AAR_ERR_INVALID, "aar_tracker_motion_bank_last: no push since creation / reset");
    if (out->struct_size < offsetof(aar_tracker_motion_info, predicted) + sizeof(int32_t))
        return set_error(AAR_ERR_INVALID, "aar_tracker_motion_bank_last: struct_size %u does not reach predicted", (unsigned)out->struct_size);
    const aar_tracker_bank::Member &m = k->mem[member];
    aar_tracker_motion_info r;
    memset(&r, 0, sizeof r);
    r.struct_size = (uint32_t)std::min<size_t>(out->struct_size, sizeof r);
    r.model = k->motion.model; r.predicted = m.last_predicted;
    memcpy(r.rel, m.last_rel, sizeof r.rel);
    motion_velocity(m.ms, r.velocity);
    r.newest_time = m.ms.tb;
    memcpy(out, &r, r.struct_size);
    return AAR_OK;
}

int aar_tracker_motion_bank_predict(aar_tracker_bank *k, int32_t member, double time, double pose[6]) {
    if (!k || !pose) return set_error(AAR_ERR_INVALID, "aar_tracker_motion_bank_predict: null argument");
    if (member < 0 || member >= k->B) return set_error(AAR_ERR_INVALID, "aar_tracker_motion_bank_predict: member = %d is outside 0 .. %d", (int)member, k->B - 1);
    if (!k->motion_on) return set_error(AAR_ERR_INVALID, "aar_tracker_motion_bank_predict: the bank has no motion model (aar_tracker_motion_bank_enable)");
    if (!k->motion_set || k->n == 0) return set_error(AAR_ERR_INVALID, "aar_tracker_motion_bank_predict: no push since creation / reset");
    const MotionState &ms = k->mem[member].ms;
    if (!std::isfinite(time) || time < ms.tb)
        return set_error(AAR_ERR_INVALID, "aar_tracker_motion_bank_predict: time = %g is not finite or lies before the newest frame's %g", time, ms.tb);
    motion_predict(ms, time, k->motion.max_dt, pose);
    return AAR_OK;
}

}  // extern "C"
