// Kernels of the Initializer (libs/initializer.cpp) and of the square-marker pose solver it calls, aruco::solvePnP_
// (3rdparty/aruco/aruco/ippe.cpp:118-223).  gfx950 only; no CPU path.
//
//   k_ippe          one thread per detection: undistort -> homography of the square -> the two IPPE rotations -> translations ->
//                   float reprojection errors -> float-rounded 4x4 poses.  Streaming: 32 B in, ~270 B out per detection.
//   k_pair_cands    one thread per candidate of a camera-pair / marker-pair set: (T, T1^-1, T2^-1) of
//                   fill_transformation_sets (:95-125) from two stored poses.  Streaming.
//   k_object_cands  the same for fill_transformation_set (:73-93), the per-frame sets of init_object_transforms.
//   k_vote          find_best_transformation (:151-193): cost_i = sum_j sum_corners |p - T2inv_j T_i T1inv_j p|.  The n^2 part:
//                   one wavefront per 64 candidates i of a set, T_i in registers, the j-side (24 doubles) read through the
//                   scalar cache because it is uniform across the wavefront; ~160 fp64 operations per (i,j): VALU-bound.
//
// All matrices are the 3x4 top of the reference's 4x4 CV_64F matrices (bottom row 0 0 0 1 stays exact under products and
// inverses), row-major.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cfloat>
#include <cstring>
#include <cmath>
#include <limits>
#include <vector>

#include "../host/init_device.h"
#include "hostcopy.h"
#include "ippe_vote.hpp"

namespace aar {

// ---------------------------------------------------------------------------------------------------------------------
// IPPE (the arithmetic: ippe_vote.hpp).  Contraction is off there: the float error is a chain of individually rounded operations
// (ippe.cpp:289-321), and the double part then rounds like the reference's scalar code as well.
// ---------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(64) k_ippe(long long n, const float *__restrict__ uv, const int *__restrict__ det_cam,
                                             const CamTab *__restrict__ cams, float hf, double *__restrict__ poses,
                                             float *__restrict__ e1, float *__restrict__ e2, float *__restrict__ uvK) {
    const long long d = (long long)blockIdx.x * 64 + threadIdx.x;
    if (d >= n) return;
    float raw[8], q[8], pk[8];
#pragma unroll
    for (int i = 0; i < 8; i++) raw[i] = uv[8 * d + i];
    d_undistort4(raw, cams[det_cam[d]], q, pk);
#pragma unroll
    for (int i = 0; i < 8; i++) uvK[8 * d + i] = pk[i];
    float ea, eb;
    d_ippe_square(hf, q, poses + (2 * d) * 12, poses + (2 * d + 1) * 12, ea, eb);
    e1[d] = ea;
    e2[d] = eb;
}

__global__ void __launch_bounds__(256) k_pair_cands(long long n, int type, const int *__restrict__ ca, const int *__restrict__ cb,
                                                    const double *__restrict__ poses, double h, double *__restrict__ Tc,
                                                    double *__restrict__ BJ) {
    const long long k = (long long)blockIdx.x * 256 + threadIdx.x;
    if (k >= n) return;
    const Aff P1 = aff_load(poses + 12LL * ca[k]), P2 = aff_load(poses + 12LL * cb[k]);
    if (type == 0) {  // cameras: T = P2 * P1^-1, T1_inv = P1, T2_inv = P2^-1
        const Aff P2i = aff_inv(P2);
        aff_store(Tc + 12 * k, aff_mul(P2, aff_inv(P1)));
        store_jside(BJ + 24 * k, P1, P2i, h);
    } else {          // markers: T = P2^-1 * P1, T1_inv = P1^-1, T2_inv = P2
        const Aff P2i = aff_inv(P2);
        aff_store(Tc + 12 * k, aff_mul(P2i, P1));
        store_jside(BJ + 24 * k, aff_inv(P1), P2, h);
    }
}

__global__ void __launch_bounds__(256) k_object_cands(long long n, const int *__restrict__ cpose, const int *__restrict__ ccam,
                                                      const int *__restrict__ cmk, const double *__restrict__ poses,
                                                      const double *__restrict__ Tcr, const double *__restrict__ Tmr, double h,
                                                      double *__restrict__ Tc, double *__restrict__ BJ) {
    const long long k = (long long)blockIdx.x * 256 + threadIdx.x;
    if (k >= n) return;
    const Aff T_mc = aff_load(poses + 12LL * cpose[k]);
    object_cand(T_mc, aff_load(Tcr + 12LL * ccam[k]), aff_load(Tmr + 12LL * cmk[k]), h, Tc + 12 * k, BJ + 24 * k);
}

// generic entry (aar_vote_transforms): j-side records from explicit T1_inv / T2_inv
__global__ void __launch_bounds__(256) k_prep_jside(long long n, const double *__restrict__ A, const double *__restrict__ B,
                                                    double h, double *__restrict__ BJ) {
    const long long k = (long long)blockIdx.x * 256 + threadIdx.x;
    if (k >= n) return;
    store_jside(BJ + 24 * k, aff_load(A + 12 * k), aff_load(B + 12 * k), h);
}

// work item: candidates [i0, i0+64) of the set [begin, end)
__global__ void __launch_bounds__(64) k_vote(const int4 *__restrict__ items, const double *__restrict__ Tc,
                                             const double *__restrict__ BJ, double h, double *__restrict__ cost) {
    const int4 it = items[blockIdx.x];
    const int begin = it.x, end = it.y;
    const int i = it.z + (int)threadIdx.x;
    const int il = i < end ? i : end - 1;
    double T[12];
#pragma unroll
    for (int k = 0; k < 12; k++) T[k] = Tc[12LL * il + k];
    const double px[4] = {-h, h, h, -h}, py[4] = {h, h, -h, -h};
    double acc = 0;
#pragma unroll 1
    for (int j = begin; j < end; j++) {
        const double *__restrict__ b = BJ + 24LL * j;   // uniform across the wavefront: scalar loads
        acc += vote_term(T, b, px, py);
    }
    if (i < end) cost[i] = acc;
}

__global__ void __launch_bounds__(256) k_gather12(int n, const int *__restrict__ idx, const double *__restrict__ src,
                                                  double *__restrict__ dst) {
    const int k = blockIdx.x * 256 + threadIdx.x;
    if (k >= n * 12) return;
    const int s = k / 12, e = k - s * 12;
    dst[k] = idx[s] >= 0 ? src[12LL * idx[s] + e] : 0.0;
}

// ---------------------------------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------------------------------
template <class T>
struct DevBuf {
    T *p = nullptr;
    hipError_t alloc(size_t n) { return hipMalloc((void **)&p, sizeof(T) * (n ? n : 1)); }
    hipError_t upload(const T *h, size_t n) {
        hipError_t e = alloc(n);
        if (e == hipSuccess && n) e = (hipError_t)h2d(p, h, sizeof(T) * n, nullptr);   // (through page-locked staging: hostcopy.h)
        return e;
    }
    ~DevBuf() { if (p) (void)hipFree(p); }
};

struct InitDevice {
    int32_t device_id = 0;
    double *poses = nullptr;   // [2 * n_det][12]
    int64_t n_poses = 0;
    ~InitDevice() { if (poses) (void)hipFree(poses); }
};

static int hip_fail(const char *what, hipError_t e) { return set_error(AAR_ERR_HIP, "%s: %s", what, hipGetErrorString(e)); }

#define HIPCHK(expr, what)                                  \
    do {                                                    \
        hipError_t e__ = (expr);                            \
        if (e__ != hipSuccess) return hip_fail(what, e__);  \
    } while (0)

static int select_device(int32_t device_id) {
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
        return set_error(AAR_ERR_NO_DEVICE, "no HIP device available; this library has no CPU path");
    if (device_id < 0 || device_id >= ndev) return set_error(AAR_ERR_INVALID, "device_id %d out of range (%d devices)", device_id, ndev);
    if (hipSetDevice(device_id) != hipSuccess) return set_error(AAR_ERR_HIP, "hipSetDevice failed");
    return AAR_OK;
}

int initdev_create(int32_t device_id, InitDevice **out) {
    if (int rc = select_device(device_id)) return rc;
    *out = new InitDevice;
    (*out)->device_id = device_id;
    return AAR_OK;
}

void initdev_destroy(InitDevice *d) { delete d; }

int initdev_ippe(InitDevice *D, const aar_cam_model *cams, int32_t n_cams, float marker_size, int64_t n, const float *uv,
                 const int32_t *det_cam, float *e1, float *e2, float *uv_undistorted) {
    if (D->poses) { (void)hipFree(D->poses); D->poses = nullptr; }
    D->n_poses = 2 * n;
    HIPCHK(hipMalloc((void **)&D->poses, sizeof(double) * 12 * (size_t)(D->n_poses ? D->n_poses : 1)), "hipMalloc(poses)");
    if (n == 0) return AAR_OK;
    std::vector<CamTab> tab((size_t)n_cams);
    for (int c = 0; c < n_cams; c++) {
        for (int i = 0; i < 9; i++) tab[c].K[i] = cams[c].K[i];
        for (int i = 0; i < AAR_MAX_DIST; i++) tab[c].k[i] = i < cams[c].n_dist ? cams[c].dist[i] : 0.0;
    }
    DevBuf<CamTab> d_tab;
    DevBuf<float> d_uv, d_e1, d_e2, d_uvK;
    DevBuf<int> d_cam;
    HIPCHK(d_tab.upload(tab.data(), tab.size()), "upload(cameras)");
    HIPCHK(d_uv.upload(uv, 8 * (size_t)n), "upload(corners)");
    HIPCHK(d_cam.upload(det_cam, (size_t)n), "upload(det_cam)");
    HIPCHK(d_e1.alloc((size_t)n), "hipMalloc");
    HIPCHK(d_e2.alloc((size_t)n), "hipMalloc");
    HIPCHK(d_uvK.alloc(8 * (size_t)n), "hipMalloc");
    hipLaunchKernelGGL(k_ippe, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, 0, (long long)n, d_uv.p, d_cam.p, d_tab.p,
                       marker_size / 2.0f, D->poses, d_e1.p, d_e2.p, d_uvK.p);
    HIPCHK(hipGetLastError(), "k_ippe");
    HIPCHK((hipError_t)d2h(e1, d_e1.p, sizeof(float) * n, nullptr), "download(e1)");
    HIPCHK((hipError_t)d2h(e2, d_e2.p, sizeof(float) * n, nullptr), "download(e2)");
    HIPCHK((hipError_t)d2h(uv_undistorted, d_uvK.p, sizeof(float) * 8 * n, nullptr), "download(corners)");
    return AAR_OK;
}

// vote every set of device-resident candidates; first minimum per set (NaN never wins, as `curr_error < min_error`)
static int vote_sets(int64_t n_cand, const double *Tc, const double *BJ, int64_t n_sets, const int64_t *set_begin,
                     double marker_size, int64_t *best, double *weight, double *best_T, double *cost_out) {
    std::vector<int4> items;
    for (int64_t s = 0; s < n_sets; s++)
        for (int64_t i0 = set_begin[s]; i0 < set_begin[s + 1]; i0 += 64)
            items.push_back(make_int4((int)set_begin[s], (int)set_begin[s + 1], (int)i0, 0));
    std::vector<double> cost((size_t)n_cand);
    if (!items.empty()) {
        DevBuf<int4> d_items;
        DevBuf<double> d_cost;
        HIPCHK(d_items.upload(items.data(), items.size()), "upload(vote items)");
        HIPCHK(d_cost.alloc((size_t)n_cand), "hipMalloc(cost)");
        hipLaunchKernelGGL(k_vote, dim3((unsigned)items.size()), dim3(64), 0, 0, d_items.p, Tc, BJ, marker_size / 2, d_cost.p);
        HIPCHK(hipGetLastError(), "k_vote");
        HIPCHK((hipError_t)d2h(cost.data(), d_cost.p, sizeof(double) * n_cand, nullptr), "download(cost)");
    }
    if (cost_out && n_cand) memcpy(cost_out, cost.data(), sizeof(double) * n_cand);
    std::vector<int> bidx((size_t)n_sets);
    for (int64_t s = 0; s < n_sets; s++) {
        double mn = std::numeric_limits<double>::max();
        int64_t at = -1;
        for (int64_t i = set_begin[s]; i < set_begin[s + 1]; i++)
            if (cost[i] < mn) { mn = cost[i]; at = i; }
        best[s] = at < 0 ? -1 : at - set_begin[s];
        if (weight) weight[s] = at < 0 ? 0.0 : mn;
        bidx[s] = (int)at;
    }
    if (best_T && n_sets) {
        DevBuf<int> d_idx;
        DevBuf<double> d_out;
        HIPCHK(d_idx.upload(bidx.data(), bidx.size()), "upload(best)");
        HIPCHK(d_out.alloc(12 * (size_t)n_sets), "hipMalloc(best_T)");
        hipLaunchKernelGGL(k_gather12, dim3((unsigned)((12 * n_sets + 255) / 256)), dim3(256), 0, 0, (int)n_sets, d_idx.p, Tc, d_out.p);
        HIPCHK(hipGetLastError(), "k_gather12");
        HIPCHK((hipError_t)d2h(best_T, d_out.p, sizeof(double) * 12 * n_sets, nullptr), "download(best_T)");
    }
    return AAR_OK;
}

static int check_sets(int64_t n_cand, int64_t n_sets, const int64_t *set_begin) {
    if (n_cand < 0 || n_sets < 0 || n_cand >= (1LL << 31) - 64) return set_error(AAR_ERR_INVALID, "vote: bad candidate count");
    if (n_sets > 0 && (!set_begin || set_begin[0] != 0 || set_begin[n_sets] != n_cand))
        return set_error(AAR_ERR_INVALID, "vote: set ranges must tile [0, n)");
    for (int64_t s = 0; s < n_sets; s++)
        if (set_begin[s + 1] < set_begin[s]) return set_error(AAR_ERR_INVALID, "vote: set ranges must ascend");
    return AAR_OK;
}

int initdev_pair_vote(InitDevice *D, int type, int64_t n_cand, const int32_t *a, const int32_t *b, int64_t n_sets,
                      const int64_t *set_begin, double marker_size, int64_t *best, double *weight, double *best_T) {
    if (int rc = check_sets(n_cand, n_sets, set_begin)) return rc;
    if (n_sets == 0) return AAR_OK;
    DevBuf<int> d_a, d_b;
    DevBuf<double> d_T, d_BJ;
    HIPCHK(d_a.upload(a, (size_t)n_cand), "upload(candidates)");
    HIPCHK(d_b.upload(b, (size_t)n_cand), "upload(candidates)");
    HIPCHK(d_T.alloc(12 * (size_t)n_cand), "hipMalloc(T)");
    HIPCHK(d_BJ.alloc(24 * (size_t)n_cand), "hipMalloc(j-side)");
    if (n_cand) {
        hipLaunchKernelGGL(k_pair_cands, dim3((unsigned)((n_cand + 255) / 256)), dim3(256), 0, 0, (long long)n_cand, type, d_a.p,
                           d_b.p, D->poses, marker_size / 2, d_T.p, d_BJ.p);
        HIPCHK(hipGetLastError(), "k_pair_cands");
    }
    return vote_sets(n_cand, d_T.p, d_BJ.p, n_sets, set_begin, marker_size, best, weight, best_T, nullptr);
}

int initdev_object_vote(InitDevice *D, int64_t n_cand, const int32_t *cand_pose, const int32_t *cand_cam,
                        const int32_t *cand_marker, int32_t n_cams, const double *to_root_cam, int32_t n_markers,
                        const double *to_root_marker, int64_t n_sets, const int64_t *set_begin, double marker_size,
                        int64_t *best, double *weight, double *best_T) {
    if (int rc = check_sets(n_cand, n_sets, set_begin)) return rc;
    if (n_sets == 0) return AAR_OK;
    DevBuf<int> d_p, d_c, d_m;
    DevBuf<double> d_Tcr, d_Tmr, d_T, d_BJ;
    HIPCHK(d_p.upload(cand_pose, (size_t)n_cand), "upload(candidates)");
    HIPCHK(d_c.upload(cand_cam, (size_t)n_cand), "upload(candidates)");
    HIPCHK(d_m.upload(cand_marker, (size_t)n_cand), "upload(candidates)");
    HIPCHK(d_Tcr.upload(to_root_cam, 12 * (size_t)n_cams), "upload(to_root_cam)");
    HIPCHK(d_Tmr.upload(to_root_marker, 12 * (size_t)n_markers), "upload(to_root_marker)");
    HIPCHK(d_T.alloc(12 * (size_t)n_cand), "hipMalloc(T)");
    HIPCHK(d_BJ.alloc(24 * (size_t)n_cand), "hipMalloc(j-side)");
    if (n_cand) {
        hipLaunchKernelGGL(k_object_cands, dim3((unsigned)((n_cand + 255) / 256)), dim3(256), 0, 0, (long long)n_cand, d_p.p, d_c.p,
                           d_m.p, D->poses, d_Tcr.p, d_Tmr.p, marker_size / 2, d_T.p, d_BJ.p);
        HIPCHK(hipGetLastError(), "k_object_cands");
    }
    return vote_sets(n_cand, d_T.p, d_BJ.p, n_sets, set_begin, marker_size, best, weight, best_T, nullptr);
}

}  // namespace aar

using namespace aar;

static void top3x4(const double *M16, double *m12, int64_t n) {
    for (int64_t i = 0; i < n; i++) memcpy(m12 + 12 * i, M16 + 16 * i, sizeof(double) * 12);
}

extern "C" int aar_ippe_square(double marker_size, const aar_cam_model *cam, int64_t n, const float *uv, double *T1, double *err1,
                               double *T2, double *err2, int32_t device_id) {
    if (!cam || n < 0 || (n > 0 && (!uv || !T1 || !T2 || !err1 || !err2)) || cam->n_dist < 0 || cam->n_dist > AAR_MAX_DIST)
        return set_error(AAR_ERR_INVALID, "aar_ippe_square: bad argument");
    InitDevice *D = nullptr;
    if (int rc = initdev_create(device_id, &D)) return rc;
    std::vector<int32_t> dc((size_t)n, 0);
    std::vector<float> e1((size_t)n), e2((size_t)n), uvK(8 * (size_t)n);
    int rc = initdev_ippe(D, cam, 1, (float)marker_size, n, uv, dc.data(), e1.data(), e2.data(), uvK.data());
    std::vector<double> P(24 * (size_t)n);
    if (!rc && n) {
        hipError_t e = (hipError_t)d2h(P.data(), D->poses, sizeof(double) * 24 * n, nullptr);
        if (e != hipSuccess) rc = hip_fail("download(poses)", e);
    }
    initdev_destroy(D);
    if (rc) return rc;
    for (int64_t d = 0; d < n; d++) {
        for (int s = 0; s < 2; s++) {
            double *T = (s ? T2 : T1) + 16 * d;
            memcpy(T, &P[(2 * d + s) * 12], sizeof(double) * 12);
            T[12] = T[13] = T[14] = 0; T[15] = 1;
        }
        err1[d] = e1[d]; err2[d] = e2[d];
    }
    return AAR_OK;
}

extern "C" int aar_vote_transforms(double marker_size, int64_t n_sets, const int64_t *set_begin, const double *T,
                                   const double *T1inv, const double *T2inv, int64_t *best, double *weight, double *cost,
                                   int32_t device_id) {
    if (n_sets < 0 || (n_sets > 0 && (!set_begin || !best))) return set_error(AAR_ERR_INVALID, "aar_vote_transforms: bad argument");
    const int64_t n = n_sets ? set_begin[n_sets] : 0;
    if (n > 0 && (!T || !T1inv || !T2inv)) return set_error(AAR_ERR_INVALID, "aar_vote_transforms: null matrices");
    if (int rc = check_sets(n, n_sets, set_begin)) return rc;
    if (int rc = select_device(device_id)) return rc;
    if (n_sets == 0) return AAR_OK;
    std::vector<double> t12(12 * (size_t)n), a12(12 * (size_t)n), b12(12 * (size_t)n);
    top3x4(T, t12.data(), n); top3x4(T1inv, a12.data(), n); top3x4(T2inv, b12.data(), n);
    DevBuf<double> d_T, d_A, d_B, d_BJ;
    HIPCHK(d_T.upload(t12.data(), t12.size()), "upload(T)");
    HIPCHK(d_A.upload(a12.data(), a12.size()), "upload(T1inv)");
    HIPCHK(d_B.upload(b12.data(), b12.size()), "upload(T2inv)");
    HIPCHK(d_BJ.alloc(24 * (size_t)n), "hipMalloc(j-side)");
    if (n) {
        hipLaunchKernelGGL(k_prep_jside, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, 0, (long long)n, d_A.p, d_B.p,
                           marker_size / 2, d_BJ.p);
        HIPCHK(hipGetLastError(), "k_prep_jside");
    }
    return vote_sets(n, d_T.p, d_BJ.p, n_sets, set_begin, marker_size, best, weight, nullptr, cost);
}
