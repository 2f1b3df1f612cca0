// Host-callable launchers of the HIP kernels (defined in eval_kernels.hip / solve_kernels.hip).
// All pointers are device pointers unless noted.  Nothing here allocates or synchronises.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <utility>

#include "../host/plan_types.h"   // CHOL_NB, PASSB_CHUNK, ObsIdx, pack_slots: what the host-only planner shares with the kernels

namespace aar {

// CG on the explicit reduced system (spcg_kernels.hip): iteration cap (sizes the hand-over buffers: one per iteration plus the
// start-up and the final one), largest system (tiles of 96 unknowns: the six rows of an entity live in one wavefront's registers)
constexpr int SPCG_MAX_IT = 128, SPCG_BUFS = SPCG_MAX_IT + 2, SPCG_MAX_NT = 14;
constexpr int SPCG_MASK_WORDS = (16 * SPCG_MAX_NT + 63) / 64;   // 64-bit words of the fixed-entity mask in k_spcg's arguments (16 entities per tile)
constexpr int SPCG_STAGE_MAX_NT = 5;  // k_spcg<NT, false> reads its rows of S in 16-byte pieces through the LDS (9 NT loads of 4 registers in flight per lane) up to this many tiles: at six the kernel starts to spill scalar registers
// default cap by system size: up to four tiles the direct chain (<= 120 us) is cheaper than a CG solve of more than ~64 iterations; larger systems' chains cost 200-500 us
inline int spcg_default_cap(int nT) { return nT <= 4 ? 64 : SPCG_MAX_IT; }
// Default forcing terms of the inexact solvers (include/aar.h: aar_solver_options.pcg_eta; DESIGN.md section 12, profiles/r05_eta_pose_sweep.txt).  Chosen for the
// final POSES: with these the poses of a run agree with the direct solver's to ~2e-6 (rotation-matrix entries) / ~1e-6 m at configs 3-5 -- 100x closer than the
// direct path is to the reference-faithful CPU run (analytic against central-difference Jacobian), 1000x closer than the reference's own last LM step moves them.
// Measured, uniform eta -> largest pose difference against the direct run (config 3, SPCG): 0.02 -> 2e-4, 3e-3 -> 2e-5, 1e-3 -> 1e-5, 3e-4 -> 2e-6, 1e-4 -> 6e-7;
// (config 5, PCG): 0.1 -> 9e-5, 0.03 -> 2e-5, 0.01 -> 5e-6, 3e-3 -> 1e-6.  A loose-then-tight SEQUENCE buys nothing at equal cost: the early steps' errors along
// weakly determined directions are never corrected by the later ones (round 4's 0.1 -> 0.02 sequence: 6e-4), so the default is ONE forcing term.
constexpr int PCG_NY = 16;   // width of the PCG kernels' barrier tree (pcg_kernels.hip, grid_hop_tree): 256 workgroups on ONE address serialise at ~60 ns each: 15 us per hop
constexpr int PCG_NYV = 2;   // k_pcgf: partial y vectors (workgroup wg adds into vector wg % PCG_NYV; every reader adds them up)
constexpr int PCG_HOP_WORDS = (2 * PCG_NY + 1) * 16;   // k_pcgf's barrier tree: PCG_NY first-level counters, one second-level counter, PCG_NY flags (64 bytes apart)
constexpr double PCG_W32_MIN_ETA = 1e-4;   // k_pcgf reads the fp32 copy of W only at forcing terms from here up (pcg_kernels.hip, launch_pcg)
constexpr double SPCG_ABS_TOL_DEFAULT = 2e-5, PCG_ABS_TOL_DEFAULT = 5e-5;   // (measured: free for SPCG at configs 3-4; PCG at config 5: 5e-5 +3 % CG iterations, 2e-5 +15 %)
constexpr double SPCG_ETA_DEFAULT = 3e-4, SPCG_ETA_LOOSE_DEFAULT = 0.0, PCG_ETA_DEFAULT = 5e-3, PCG_ETA_LOOSE_DEFAULT = 0.0;
inline int spcg_stride(int n_pad) { return 8 * (n_pad / 6); }   // doubles per hand-over buffer: one 64-byte record per entity


#ifndef SPCG_PRE
#define SPCG_PRE 0   // s_sleep units (64 cycles) between a wavefront's publish and its first poll of a hand-over (measured: 0 is best, profiles/r04_spcg_probe.txt)
#endif

// Kernel ids for the optional per-launch timing hooks (aar_get_kernel_times)
enum KernelId { KID_UNPACK = 0, KID_RESIDUAL, KID_PASSA, KID_PASSB, KID_MAXDIAG, KID_FRAME_INV, KID_SCHUR, KID_LDL_DIAG,
                KID_LDL_TRSM, KID_LDL_UPDATE, KID_LDL_BACKSOLVE, KID_BACKSUB, KID_REDUCE, KID_LDL_PANEL, KID_PCG, KID_SPCG, KID_SPCG_PRE, KID_PRIOR, KID_COUNT };

struct LaunchHook {  // called around every kernel launch when profiling is on
    void (*pre)(void *ctx, int kid) = nullptr;
    void (*post)(void *ctx, int kid) = nullptr;
    void *ctx = nullptr;
};

struct DeviceProblem {
    // sizes
    int C = 0, M = 0, A = 0;          // cameras, markers, shared entities A = C + M (+ C intrinsics entities when intr)
    int intr = 0;                     // optimize_cam_intrinsics: entity C + M + c = (fx, cx, fy, cy, -, -) of camera c, its row = K
    int F = 0;                        // local frames
    int64_t N = 0;                    // local observations
    int n = 0, n_pad = 0, nT = 0;     // reduced system: n = 6A, padded to a multiple of CHOL_NB, tiles
    int total_slots = 0, max_kf = 0;  // sum / max of distinct shared entities per frame
    int n_chunks = 0, n_swork = 0;
    int res_f32 = 1;
    float huber = -1.f;               // Huber delta of the residual weights (< 0: plain residuals)
    double half_size = 0;             // (double)((float)marker_size / 2.f)
    // constant problem data
    double *K = nullptr;              // [C][9]
    ObsIdx *a_idx = nullptr;          // ordering A = reference order (frame, camera, detection order)
    float *a_uv = nullptr;            // [N][8]
    int32_t *frame_obs_start = nullptr;   // [F+1]
    int32_t *frame_stride = nullptr;      // [F] pass A (wrench form): lane i of a frame's workgroup starts at observation (i * stride) mod n, stride coprime with n
    int32_t *fslot_start = nullptr;       // [F+1] first W block of each frame
    int32_t *fslot_ent = nullptr;         // [total_slots] shared entity of each W block (ascending inside a frame)
    ObsIdx *b_idx = nullptr;          // ordering B = (camera, marker, frame)
    float *b_uv = nullptr;
    int32_t *chunk_start = nullptr;   // [n_chunks+1] into ordering B; a chunk never spans two (camera, marker) runs
    int32_t *ent_fixed = nullptr;     // [A] 1 = root, non-optimised group or fixed by the caller (aar_problem_constraints)
    int frames_fixed = 0;
    // Schur work list: item w handles pairs [sw_begin[w], sw_end[w]) of entity sw_ent[w]
    int32_t *sw_ent = nullptr, *sw_begin = nullptr, *sw_end = nullptr;
    int4 *pair_rec = nullptr;             // (entity, frame) incidence, grouped by entity: {frame, W block, first W block of the frame, 0}
    // Schur work list of the MFMA kernel (many shared entities): item w = block (16 dense entities sm_ga[w]) x (32 dense entities
    // sm_gb[w]) of S over the frames sm_frames[sm_fb[w] .. sm_fe[w])
    int n_smwork = 0;
    int32_t *sm_ga = nullptr, *sm_gb = nullptr, *sm_fb = nullptr, *sm_fe = nullptr, *sm_frames = nullptr;
    // ... which reads DENSE per-frame panels: dense entity 0 = the frame's gradient g_f (a pseudo entity whose block row 0 is g_f: its
    // column of S is the Schur part of the right-hand side), 1.. = the shared entities that are seen at all, MOST FREQUENT FIRST
    // (ties ascending; k_schur_mfma stores a pair transposed where the real entity order is the other way round); Ad = their
    // number padded to a multiple of 32.  Blocks of absent (entity, frame) pairs are zero ONCE and for all (the visibility pattern
    // never changes), k_schur_fill only rewrites the present ones.
    int Ad = 0;
    int32_t *slot_dense = nullptr;        // [total_slots] dense entity of every W block
    int32_t *slot_frame = nullptr;        // [total_slots] frame of every W block
    int32_t *dense_ent = nullptr;         // [Ad] shared entity of a dense index (-1: the pseudo entity / padding)
    double *Wd = nullptr, *Yd = nullptr;  // [F][Ad][36] W_af and W_af (V_f + mu I)^-1
    int dense_from_passA = 1;             // pass A writes them itself whenever it inverts V_f for a predicted damping (AAR_DENSE_FROM_PASSA=0: always k_schur_fill)
    // AAR_DETERMINISTIC=1: every sum that the default path leaves to fp64 atomics (whose order changes from run to run) is taken
    // in a FIXED order instead -- pass B writes per-chunk partials that a second kernel adds up chunk-ascending, the Schur kernel
    // (always the output-stationary one, one wavefront per work item) writes per-item row panels that a second kernel adds up
    // frame-ascending, pass A runs one wavefront per frame.  Two runs of the same problem then give the same bits.
    int deterministic = 0;
    double *pb_part = nullptr;            // [n_chunks][pb_stride] per-chunk sums of pass B (90 values, + 62 with intrinsics)
    int pb_stride = 0, n_pbr = 0;
    // reduction items of pass B: item i adds up the chunks pbr_chunk[pbr_start[i] .. pbr_start[i+1]) (ascending) for camera pbr_a
    // (kind 0), marker entity pbr_a (kind 1) or the pair (camera pbr_a, marker entity pbr_b) (kind 2)
    int32_t *pbr_start = nullptr, *pbr_chunk = nullptr, *pbr_kind = nullptr, *pbr_a = nullptr, *pbr_b = nullptr;
    double *sp_part = nullptr;            // per Schur work item: its row panel [(a+1)*36] | its 6 rhs entries | 2 idle
    int64_t *sp_off = nullptr;            // [n_swork] first double of the item's record
    int32_t *se_start = nullptr, *se_items = nullptr;   // [A+1], [n_swork]: the work items of every entity, frame-ascending
    // AAR_SOLVER=pcg (opt-in, pcg_kernels.hip): the reduced system solved by preconditioned CG through the frame blocks
    int use_pcg = 0, pcg_grid = 0, pcg_max_it = 200;
    double pcg_eta = 0.1;                 // |r| <= eta |b| stops an inner solve of a LATE LM step (aar_solver_options.pcg_eta)
    // the inexact solvers' forcing SEQUENCE when AUTO chose them and the caller left the forcing term at its default: while the LM is still far from its stopping rule (the last
    // accepted step took more than pcg_eta_switch of the error away) the inner solve stops at pcg_eta_loose, afterwards at pcg_eta -- the steps that decide
    // the stopping rule are solved as tightly as before (profiles/r04_pcg_eta_sweep.txt).  pcg_eta_now is what the next launch uses.
    double pcg_eta_loose = 0.0, pcg_eta_switch = 0.01, pcg_eta_now = 0.1;
    // ... and an ABSOLUTE one beside the relative forcing term (both must hold): the error an inner solve leaves in the step, in the units of the pose vector (radians / metres).
    // The relative term alone lets a solve stop while the step is still large in absolute terms -- far starts, a tiny initial damping (tau = 1e-6: poses 4e-3 off): there the
    // absolute term keeps the CG going (or sends the try to the direct chain through the iteration cap).  Both solvers: r^T M^-1 r <= eps^2 mu (M = the block-Jacobi preconditioner).
    double pcg_abs_tol = SPCG_ABS_TOL_DEFAULT;
    int pcg_n_items = 0;                  // work items of the entity-side passes (pcg_kernels.hip): ranges of one entity's incidences in pair_rec
    int32_t *pcg_it_ent = nullptr, *pcg_it_begin = nullptr, *pcg_it_end = nullptr, *pcg_ent_item_start = nullptr;
    double *pcg_ws = nullptr;             // items' shares [n_items][28] | t [6F]
    int32_t *pcg_counter = nullptr;       // [0..1] grid-barrier counters (alternating), [2] iterations of the last solve, [3] running total
    mutable int pcg_parity = 0;
    int n_cus = 256;                      // compute units of the device (hipDeviceProp_t::multiProcessorCount)
    mutable int want_w64 = 0;             // aar_eval_normal_equations: pass A writes the fp64 W blocks even where the solver only reads the fp32 copy (Blocks::Wf)
    int pcg_fused = 1;                    // AAR_PCG_FUSED=0: k_pcg (two passes over W and two hand-overs per iteration) instead of k_pcgf
    int pcg_rank0 = 1;                    // this rank adds the terms of the sharded PCG's set-up that must enter ONCE (the damping of the coarse operator)
    int pcg_resident = 1;                 // AAR_PCG_RESIDENT=0: k_pcgf streams every W block once per CG iteration (1: the first round of every wavefront's first frame stays in registers for the solve -- fp32 blocks; both rounds with fp64 blocks, whose kernel has 512 registers per lane)
    int pcg_e_every = 1;                  // AAR_PCG_E_EVERY: k_pcgf forms the coarse operator's Z^T S Z every this-many solves of an LM run and keeps it in between (the damping's mu Z^T Z is always today's); 1: every solve; set by size at problem creation (3 from 300 000 (entity, frame) pairs)
    mutable int pcg_e_age = 0;            // solves since E was formed (0: the next one forms it; reset where an LM run starts)
    int pcg_coarse = 1, pcg_coarse_from = 8;   // AAR_PCG_COARSE=0 / AAR_PCG_COARSE_FROM: k_pcgf's coarse space (the groups' rigid-motion modes) joins when the previous solve of the LM run took this many iterations
    int32_t *up_start = nullptr, *up_ent = nullptr;   // [A + 1], [..]: entity -> the OTHER entities whose block of U can be non-zero (seen together in an observation); the CG operator skips the rest
    double *pcg_yg = nullptr;             // k_pcgf: y [3][PCG_NYV][n_pad] (rotating; PCG_NYV partial vectors) | the set-up's sums [A][28]
    int32_t *pcg_hop = nullptr;           // k_pcgf: [2][PCG_HOP_WORDS] barrier tree (pcg_kernels.hip, grid_hop_tree), by launch parity
    // solver spcg (spcg_kernels.hip): CG on the explicit Schur complement, one wavefront per shared entity
    int use_spcg = 0, spcg_max_it = 64;
    int spcg_spread = 8;                  // AAR_SPCG_SPREAD=1: every workgroup of the grid works (the wavefronts then sit on all XCDs and hand over through memory)
    int spcg_coarse = 1;                  // AAR_SPCG_COARSE=0: block-Jacobi only (the A/B reference of the two-level preconditioner)
    int spcg_coarse_from = 12;            // AAR_SPCG_COARSE_FROM: the coarse space joins once a solve of the LM run has taken this many CG iterations (0: from the first solve)
    mutable int spcg_coarse_on = 0;       // the next k_spcg launch carries the coarse space (damped_try decides; sticky within an LM run)
    double *spcg_pre = nullptr;           // workspace of k_spcg_pre (spcg_pre_doubles): augmented rows | right-hand side | inverse blocks | Z | (A Z)^T | shares | counter
    mutable int spcg_pre_epoch = 0;       // launches of k_spcg_pre (its arrival counter is monotonic)
    int spcg_root_c = -1, spcg_root_m = -1, spcg_n_free = 0;   // the fixed entity of each group whose slot carries the group's rigid-motion unknowns (-1: none); free entities
    unsigned long long spcg_fixed[SPCG_MASK_WORDS] = {~0ull, ~0ull, ~0ull, ~0ull};   // ent_fixed and the padding entities as bits (spcg_build_fixed_mask: whenever ent_fixed is set)
    int spcg_test_drop = -1;              // test hook (AAR_SPCG_TEST_DROP=entity): that entity's wavefront never shows up -> every hand-over times out -> flag 4 -> direct chain
    double *spcg_ws = nullptr;            // [2][SPCG_BUFS][spcg_stride(n_pad)] hand-over slots (sentinel-filled when idle)
    int32_t *spcg_iters = nullptr;        // [0] iterations of the last solve, [1] running total, [2] solves, [3] solves that hit the cap (flag 8)
    mutable int spcg_parity = 0;
    // ... with frames sharded over ranks: this rank's set-up share [A][28] (all-reduced), Minv [A][36], x | r | p | scalars [3 n + 8],
    // this rank's partial y [n] (all-reduced per iteration), mapped host record {done, iterations, -, sequence}
    double *pcgd_setup = nullptr, *pcgd_minv = nullptr, *pcgd_state = nullptr, *pcgd_y = nullptr, *pcgd_host = nullptr;
    // tuning switches (environment, read when THE PROBLEM is created -- aar_problem_create_ex -- so that two problems of one process may differ;
    // defaults are the measured optima)
    struct Tuning {
        int fused_panel = 3;       // AAR_FUSED_PANEL: block columns with at most this many tiles below the diagonal take k_ldl_panel
        int bs_rides = 1;          // AAR_BS_RIDES=0: the back-substitution of 2-3 tile systems as its own chained launch
        int lookahead = 1;         // AAR_LDL_LOOKAHEAD=0: tall block columns launch k_ldl_update
        int passA_variant = 0;     // AAR_PASSA_VARIANT (test hook): 641 / 642 / 644 / 1284 force one of pass A's four production workgroup shapes (threads, corners per lane)
        int passAB_occ2 = -1;       // AAR_PASSAB_OCC2=0 / 1: the merged observation passes capped at 256 registers (two wavefronts per SIMD); -1: when their workgroups exceed one round of the chip's slots
        int passA_wrench = 1;      // AAR_PASSA_WRENCH=0: pass A in its row form (three Jacobian blocks per row, 100 accumulators per lane) -- the A/B reference of the wrench form
        int pack_system = -1;      // AAR_PACK_SYSTEM=0/1: the reduced system travels as it lies / as the packed triangle (default: by size)
        int init_headstart = 1;    // AAR_INIT_HEADSTART=0: the first step's frame inverses and Schur complement wait for the host to have read mu_0
    } tune;
    // state: everything that depends on a pose vector exists twice (index 0/1 = the two pose buffers), so that the
    // blocks of a trial point can be built while those of the current point are still needed for a mu retry
    double *z[2] = {nullptr, nullptr};    // [6A + 6F] pose vectors
    double *ent[2] = {nullptr, nullptr};  // [(A+F)][ENT_STRIDE]
    struct Blocks {
        double *V = nullptr, *gf = nullptr;   // [F][36], [F][6]
        double *W = nullptr;                  // [total_slots][36]   W_af (rows: entity params, cols: frame params)
        float *Wf = nullptr;                  // PCG (k_pcgf, fp32 operator): the same blocks in fp32, per frame piece-major -- float4 piece q (entries 4q .. 4q+3 of the
                                              // row-major block) of the frame's slot j at float4 index (fslot_start[f] * 9 + q k_f + j) -- written by pass A beside W
        double *Vinv = nullptr, *hf = nullptr;// (V_f + mu I)^-1, (V_f + mu I)^-1 g_f
        double *S = nullptr;                  // [n_pad*n_pad] row-major lower triangle: shared blocks (pass B), then minus
                                              // the Schur terms, then (in place) its LDL^T factor
        double *rhs = nullptr;                // [n_pad] Schur part of the right-hand side, then z = D^-1 L^-1 b
        double *g0 = nullptr;                 // [n_pad] shared part of B = -J^T r (kept for the gain denominator)
        double *tail = nullptr;               // [8] right behind g0: the step's scalars of THIS rank, so that on the multi-GPU path
                                              // they travel in the same all-reduce as the next step's S | rhs | g0
    } blk[2];
    double *Dfac = nullptr;               // [nT][NB*NB] factored diagonal tiles (unit L below, D on the diagonal)
    double *Linv16 = nullptr;             // [nT][6][16*16] inverses of the 16x16 diagonal sub-blocks of every L_ss
    double *Lp = nullptr;                 // [nT][n_pad][NB] block columns of L written by the fused panel kernel (stages with <= 2 tiles below the diagonal)
    double *zf = nullptr;                 // [n_pad] forward-substituted right-hand side of those stages
    double *delta_s = nullptr;            // [n_pad]
    int32_t *bs_flags = nullptr;          // [nT] k_ldl_backsolve: flag[s] == bs_epoch <=> x_s of the current launch is in memory
    mutable int bs_epoch = 0;
    double *err_part = nullptr;           // [max(F, residual_blocks)] partial sums of squared residuals
    double *lin_part = nullptr;           // [F+1][2] per-frame ( |delta_f|^2 , delta_f . g_f ), last = shared part
    double *scal = nullptr;               // [8] reduced scalars
    // host-visible (pinned, mapped) result record the reduction kernel publishes: [0..7] scalars, [8] flags, [9] sequence
    double *host_result = nullptr;        // device pointer to the mapped host record (10 x 8 bytes)
    int32_t *flags = nullptr;             // [4] device error flags (0: non-positive pivot)
    double *r_out = nullptr;              // optional [8N]
    // pose priors (prior_kernels.hip): every rank holds them, only rank 0 (prior_rank0) adds them into the system
    int n_prior = 0, prior_rank0 = 1;
    int32_t *prior_ent = nullptr;         // [n_prior] shared entity
    double *prior_dat = nullptr;          // [n_prior][PRIOR_DAT] x6 | information matrix
    double *prior_out = nullptr;          // [n_prior][8] e | cost | 0, then the summed cost
    // relative pose priors between two cameras / two markers (pair_prior_kernels.hip): held and added as the pose priors are
    int n_pair = 0, n_pair_el = 0, n_pair_items = 0;
    int32_t *pair_ends = nullptr;         // [n_pair][4] entity a, entity b, 1 = both ends free, 0
    double *pair_dat = nullptr;           // [n_pair][PRIOR_DAT] x6_rel | information matrix
    int32_t *pair_el_ent = nullptr, *pair_el_start = nullptr, *pair_el_item = nullptr;   // free end entities -> their (pair, side) items, ascending
    double *pair_rec_ws = nullptr;        // [n_pair][54] the diagonal contributions between the kernel's two phases
    double *pair_out = nullptr;           // [n_pair][8] e | cost | 0, then the summed cost
    LaunchHook hook;
};

// Opt `kernel` in to `bytes` of dynamic LDS per workgroup on the current device (gfx950: up to 160 KiB per CU).  One process-wide,
// mutex-guarded table per (device, kernel) holds what was granted: the attribute is only ever raised (from 48 KiB), so no problem or
// thread lowers it under another's live launches (ba_capi.hip).
void raise_dynamic_lds(const void *kernel, size_t bytes);
// every launch with dynamic LDS: the opt-in, then the launch with the same arguments
template <typename... Params, typename... Args>
inline void launch_lds(void (*kernel)(Params...), dim3 grid, dim3 block, size_t lds, hipStream_t st, Args &&...args) {
    raise_dynamic_lds(reinterpret_cast<const void *>(kernel), lds);
    hipLaunchKernelGGL(kernel, grid, block, lds, st, std::forward<Args>(args)...);
}

// camera matrices: the constant table, or -- intrinsics being optimised -- the rows of the intrinsics entities of pose buffer `which`
struct KTable { const double *base; int stride; };
constexpr int ENT_STRIDE_H = 24;   // = geom.hpp's ENT_STRIDE
inline KTable k_table(const DeviceProblem &P, int which) {
    if (P.intr) return KTable{P.ent[which] + (size_t)(P.C + P.M) * ENT_STRIDE_H, ENT_STRIDE_H};
    return KTable{P.K, 9};
}

extern volatile int g_last_kernel_id;   // the kernel id of the most recent launch of this process (diagnostics: AAR_ABORT_BACKTRACE prints it)
struct HookScope {  // RAII: pre/post around one launch
    const DeviceProblem &P;
    int kid;
    HookScope(const DeviceProblem &p, int k) : P(p), kid(k) { g_last_kernel_id = k; if (P.hook.pre) P.hook.pre(P.hook.ctx, kid); }
    ~HookScope() { if (P.hook.post) P.hook.post(P.hook.ctx, kid); }
};

// z -> ent (start of a solve, rebuilds, the residual-vector API); zero_blk >= 0: the same launch clears that block set's S | rhs | g0 and lin_part
void launch_unpack(const DeviceProblem &P, int which, hipStream_t st, int zero_blk = -1);
void launch_residual(const DeviceProblem &P, int which, double *r_out, hipStream_t st);
// pass A at z[which]: entity table, V, g_f, W, per-frame sum r^2 (err_part[f]); mu_pred >= 0 also gives Vinv, h_f for that
// damping; zero_blk >= 0 clears S, rhs, g0 of that block set (they are dead / about to be rebuilt)
void launch_passA(const DeviceProblem &P, int which, double mu_pred, int zero_blk, hipStream_t st);
void launch_passB(const DeviceProblem &P, int which, hipStream_t st);              // accumulates into blk[which].S, .g0 (must be zero); with intrinsics: their shared blocks too
// both passes in one launch (they only share the entity table ent[which], which must be complete); false = nothing launched
bool launch_passAB(const DeviceProblem &P, int which, double mu_pred, int zero_blk, hipStream_t st);
size_t passA_lds_bytes(int max_kf, int block);   // dynamic LDS of the frame-block kernel in row form (block = 64 or 256 threads)
size_t passA_wrench_lds_bytes(int max_kf, bool intr);   // ... in wrench form (the default)
void launch_maxdiag(const DeviceProblem &P, int which, hipStream_t st);            // scal[4] = max free diagonal
void launch_frame_inv(const DeviceProblem &P, int which, double mu, hipStream_t st, const double *mu_dev = nullptr, double mu_scale = 0.0);   // mu_dev: mu = mu_scale * mu_dev[0], read on the device
// S -= sign * W (V+mu I)^-1 W^T (sign -1 takes it back).  ride_seq != 0: the reduction of the step's scalars rides in the same
// launch (true is returned if it did)
// panels_ready (MFMA path): Wd / Yd already hold this block set's panels for the damping in Vinv (pass A wrote them): no k_schur_fill
bool launch_schur(const DeviceProblem &P, int which, double sign, hipStream_t st, unsigned long long ride_seq = 0, int ride_n_err = 0,
                  double *ride_scal = nullptr, bool panels_ready = false);   // ride_scal: the rider leaves the scalars there and does not publish
// damping + LDL^T + both substitutions -> delta_s
void launch_chol(const DeviceProblem &P, int which, double mu, hipStream_t st);
void launch_backsub(const DeviceProblem &P, int cur, int trial, hipStream_t st);   // z[trial] = z[cur] + delta, lin_part
void launch_pcg(const DeviceProblem &P, int which, double mu, hipStream_t st);     // AAR_SOLVER=pcg: delta_s by PCG through the frame blocks (needs Vinv, hf for mu)
size_t pcg_lds_bytes(int A, bool coarse = false);   // coarse: with the tables of k_pcgf's coarse space
int pcg_max_grid(int A, bool coarse, int cus);   // largest co-resident grid of the persistent PCG kernels at the dynamic LDS they are launched with
// solver spcg: delta_s by CG on the explicit reduced system S of block set `which` (the Schur complement for mu must have been taken; S is not modified)
void launch_spcg(const DeviceProblem &P, int which, double mu, hipStream_t st);
int spcg_resident_per_cu(int nT, bool coarse);             // occupancy query: wavefronts of k_spcg<nT> one CU holds (0: unknown)
inline bool spcg_coarse_now(const DeviceProblem &P) { return P.spcg_coarse && (P.spcg_root_c >= 0 || P.spcg_root_m >= 0); }   // this problem's k_spcg can carry the coarse space
void spcg_build_fixed_mask(DeviceProblem &P, const int32_t *ent_fixed_host);   // P.spcg_fixed from the host's copy of ent_fixed [P.n / 6]
bool spcg_fits(int nT);                                    // the system's rows fit the wavefronts' registers
size_t spcg_ws_doubles(int n_pad);
size_t spcg_pre_doubles(int n_pad);
void spcg_ws_reset(const DeviceProblem &P, hipStream_t st);   // every hand-over slot back to the sentinel (at creation, after a timed-out launch)
// the same with a communicator: set-up share -> [all-reduce] -> launches k = 0, 1, .. with an all-reduce of pcgd_y between two of them
void launch_pcgd_setup(const DeviceProblem &P, int which, double mu, hipStream_t st);
void launch_pcgd_iter(const DeviceProblem &P, int which, double mu, int k, bool last, unsigned long long publish_seq, hipStream_t st);
double *pcgd_y_of_launch(const DeviceProblem &P, int k);   // this rank's partial y of launch k: what the host all-reduces before launch k + 1
void launch_reduce_scalars(const DeviceProblem &P, int n_err, bool fold_shared, unsigned long long publish_seq, hipStream_t st,
                           double *scal_out = nullptr, int maxdiag_blk = -1);  // scal[0..2], scal[5..6] (into scal_out instead of P.scal if given);
                                                                               // maxdiag_blk >= 0: also scal[4] = max free diagonal of that block set (k_maxdiag's job)
// scal / flags -> host record; flags_reduced: the flags are decoded from src[3] (every rank's flags, all-reduced) instead of P.flags
void launch_publish(const DeviceProblem &P, unsigned long long publish_seq, hipStream_t st, const double *src = nullptr, bool flags_reduced = false);
int residual_blocks(const DeviceProblem &P);   // entries of err_part written by launch_residual
// pose priors at ent[which]: e and the costs into prior_out; add (and rank 0): J^T L J into the diagonal blocks of blk[which].S, -J^T L e into
// its g0, the summed cost into err_part[F].  Runs after pass B is complete and before anything reads S (maximum diagonal, Schur complement)
constexpr int PRIOR_DAT = 42;
void launch_prior(const DeviceProblem &P, int which, bool add, hipStream_t st);
// entries of err_part the step's error sums: the frames' and, with priors on this rank, their cost behind them
inline int n_err_terms(const DeviceProblem &P) { return P.F + (((P.n_prior > 0 || P.n_pair > 0) && P.prior_rank0) ? 1 : 0); }
// relative pose priors at ent[which], right behind launch_prior at every site: e and the costs into pair_out; add (and rank 0): the two diagonal
// blocks and the cross block of every pair into blk[which].S, -J^T L e into its g0, the summed cost into err_part[F] (added to k_prior's, if any)
void launch_pair_prior(const DeviceProblem &P, int which, bool add, hipStream_t st);
inline int n_prior_launches(const DeviceProblem &P) { return (P.n_prior ? 1 : 0) + (P.n_pair ? 1 : 0); }
// track(): every frame's own 6-DoF LM, whole loop on the device; needs ent[which] rows of the shared entities (launch_unpack)
void launch_track(const DeviceProblem &P, int which, int max_iters, double min_error, double min_step, double min_avg, double tau,
                  int32_t *iters_out, double *err_out, hipStream_t st);

// smoothed tracking (smooth_kernels.hip): the workspace of one aar_track_smooth call, carved out of one allocation
constexpr int SMOOTH_TAIL = 256;   // threads of the workgroup that finishes the cyclic reduction: levels with at most this many eliminating nodes run inside it
struct SmoothWork {
    double *z[2] = {nullptr, nullptr};     // [F][6] frame poses: the current point and the trial point
    double *delta = nullptr;               // [F][6] the damped step
    double *Dg = nullptr, *Of = nullptr;   // [F][36] H_ff, [F][36] H_{f,f+1} (row-major, rows: frame f; the last one unused)
    double *rhs = nullptr;                 // [F][6] b
    double *Dw = nullptr, *Uw = nullptr, *bw = nullptr, *Dinv = nullptr, *Ls = nullptr;   // the reduction's working copy and what its back-substitution keeps
    double *Ef[2] = {nullptr, nullptr}, *Pe[2] = {nullptr, nullptr};   // [F] data cost per frame, prior cost per pair, of the two points
    double *lin = nullptr;                 // [F][2] |delta_f|^2, delta_f . b_f
    double *lam = nullptr;                 // [F-1][2] 1 / (sigma_rot^2 dt), 1 / (sigma_trans^2 dt)
    double *rel_buf = nullptr;             // [F-1][6] storage of the expected relative motions ...
    const double *rel = nullptr;           // ... = rel_buf when the caller gave any, else NULL
    double *res = nullptr;                 // [8] the record the host reads: data cost, prior cost, |delta|^2, delta . b, max diag H, pivot flag
    int32_t *flag = nullptr;               // [1] a non-positive pivot in the last solve
};
size_t smooth_work_doubles(int F);
void smooth_work_carve(SmoothWork &w, double *base, int F);
void launch_smooth_eval(const DeviceProblem &P, int which, const SmoothWork &w, int cur, bool with_j, hipStream_t st);   // two launches
int launch_smooth_solve(const SmoothWork &w, int F, double mu, hipStream_t st);                                          // returns its launches
// the diagonal and lag-one blocks of H^-1 from what launch_smooth_solve(w, F, 0.0, st) left (smooth_cov_kernels.hip)
int launch_smooth_selinv(const SmoothWork &w, int F, double *S, double *R, hipStream_t st);                               // returns its launches
// pose and covariance block at Q > 0 query times from z [F][6], the frame times ft [F] and S, R of launch_smooth_selinv (smooth_query_kernels.hip,
// DESIGN.md section 30); cov == NULL: poses and segments only, w, S, R and flag unused.  All pointers on the device; flag zeroed by the caller
int launch_smooth_query(const SmoothWork &w, int F, const double *z, const double *ft, double sigma_rot, double sigma_trans, const double *S,
                        const double *R, int64_t Q, const double *qt, double *pose, double *cov, int32_t *seg, int32_t *flag,
                        hipStream_t st);                                                                                  // returns its launches
// the pairs' expected sufficient statistics from S, R and z[cur] (smooth_fit_kernels.hip), F >= 2: terms [F-1][4] =
// a_r, u_r, a_t, u_t and rec [8] = their sums, w.res[0], w.res[1], w.flag[0], 0; sigma_rot: the one w.lam was built with
int launch_smooth_fit_terms(const SmoothWork &w, int cur, int F, double sigma_rot, const double *S, const double *R, double *terms, double *rec,
                            hipStream_t st);                                                                              // returns its launches
// k_smooth_reduce on its own (one launch): Ef, Pe [F]; lin [F][2] or NULL; Dg [F][36] or NULL -> res [8]
void launch_smooth_reduce(const double *Ef, const double *Pe, const double *lin, const double *Dg, const int32_t *flag, int F, double *res,
                          hipStream_t st);

// smoothed tracking under the constant-velocity prior (smooth_cv_kernels.hip): H is block pentadiagonal; the solve pairs
// the frames into K = ceil(F / 2) supernodes (2k, 2k + 1) of 12x12 blocks, block tridiagonal again, and runs section 16's cyclic reduction on them
constexpr int SMOOTH_CV_T = 16;    // levels with at most this many eliminating supernodes run inside the one workgroup that finishes the reduction
struct SmoothCvWork {
    double *z[2] = {nullptr, nullptr};     // [F][6] frame poses: the current point and the trial point
    double *delta = nullptr;               // [2K][6] the damped step (the padded frame of an odd F: zeros)
    double *Dg = nullptr, *O1 = nullptr, *O2 = nullptr;   // [F][36] H_ff, H_{f,f+1}, H_{f,f+2} (row-major, rows: frame f; zeros where there is none)
    double *rhs = nullptr;                 // [F][6] b
    double *Dw = nullptr, *Uw = nullptr, *Dinv = nullptr, *Ls = nullptr;   // [K][144] the reduction's working copy and what its back-substitution keeps
    double *bw = nullptr;                  // [K][12]
    double *Ef[2] = {nullptr, nullptr}, *Pe[2] = {nullptr, nullptr};   // [F] data cost per frame, prior cost per term (entry 0: pair 0, entry F-1: 0)
    double *lin = nullptr;                 // [F][2] |delta_f|^2, delta_f . b_f
    double *lam = nullptr;                 // [F][2] of term f (entry 0: pair 0 with sigma_rot0 / sigma_trans0): 1 / (sigma_rot^2 dt_f), 1 / (sigma_trans^2 dt_f)
    double *ratio = nullptr;               // [F] r_f = dt_f / dt_{f-1} of term f
    double *res = nullptr;                 // [8] as SmoothWork::res
    int32_t *flag = nullptr;               // [1] a non-positive pivot in the last solve
};
inline int smooth_cv_nodes(int F) { return (F + 1) / 2; }
size_t smooth_cv_work_doubles(int F);
void smooth_cv_work_carve(SmoothCvWork &w, double *base, int F);
void launch_smooth_cv_eval(const DeviceProblem &P, int which, const SmoothCvWork &w, int cur, bool with_j, hipStream_t st);   // two launches
int launch_smooth_cv_solve(const SmoothCvWork &w, int F, double mu, hipStream_t st);                                          // returns its launches
int smooth_cv_solve_launches(int F);                                                                                          // ... that number, on the host
// the diagonal, lag-one and lag-two blocks of H^-1 from what launch_smooth_cv_solve(w, F, 0.0, st) left (smooth_cv_cov_kernels.hip, DESIGN.md
// section 32): area = smooth_cv_selinv_doubles(F) zeroed doubles on the device; fc, lc, l2 [F][36] each are returned as pointers into it
size_t smooth_cv_selinv_doubles(int F);
int smooth_cv_selinv_launches(int F);
int launch_smooth_cv_selinv(const SmoothCvWork &w, int F, double *area, double **fc, double **lc, double **l2, hipStream_t st);   // returns its launches
// the constant-velocity track at any time (smooth_cv_query_kernels.hip).  launch_smooth_cv_lag3: l3 [F-3][36], l3[f] =
// (H^-1)_{f,f+3}, from the area launch_smooth_cv_selinv worked on (its S and R[0] stay there); no launch below four frames.
// launch_smooth_cv_query: pose, covariance block and segment at Q > 0 query times from z [F][6], the frame times ft [F] and the blocks by lag;
// cov, start (the start poses) and step (delta_m) may be NULL.  All pointers on the device; flag zeroed by the caller; both return their launches
int launch_smooth_cv_lag3(int F, const double *area, double *l3, int32_t *flag, hipStream_t st);
int launch_smooth_cv_query(int F, const double *z, const double *ft, double sigma_rot, double sigma_trans, double sigma_rot0, double sigma_trans0,
                           const double *fc, const double *lc, const double *l2, const double *l3, int64_t Q, const double *qt, double *pose,
                           double *cov, double *start, double *step, int32_t *seg, int32_t *flag, hipStream_t st);
// the covariance between any two frames and the relative motion with its covariance (smooth_relative_kernels.hip): the
// answers of Q > 0 pairs (fa[q], fb[q]) into cross [Q][36], rel [Q][6], rcov [Q][36] from what the selected inverses left on the same stream
// (S, R of launch_smooth_selinv; the area and fc, lc, l2 of launch_smooth_cv_selinv with l3 of launch_smooth_cv_lag3).  C takes the gains
// ([F][36], [K][144]) and is written only with chained = true: some pair lies beyond the blocks that exist (lag above 1, above 3).  All
// pointers on the device; flag zeroed by the caller, raised by a non-positive pivot of a gain; both return their launches
int launch_smooth_relative(int F, const double *z, const double *S, const double *R, double *C, bool chained, int64_t Q, const int32_t *fa,
                           const int32_t *fb, double *cross, double *rel, double *rcov, int32_t *flag, hipStream_t st);
int launch_smooth_cv_relative(int F, const double *z, const double *area, const double *fc, const double *lc, const double *l2, const double *l3,
                              double *C, bool chained, int64_t Q, const int32_t *fa, const int32_t *fb, double *cross, double *rel, double *rcov,
                              int32_t *flag, hipStream_t st);
// the terms' expected sufficient statistics from fc, lc, l2 and z[cur] (smooth_cv_fit_kernels.hip), F >= 3: terms [F-1][4]
// = a_r, u_r, a_t, u_t (entry 0: pair 0), rec [8] = A_r, U_r, A_t, U_t over the terms 1 .. F-2, data cost, prior cost, pivot flag, u_0;
// returns its launches
int launch_smooth_cv_fit_terms(const SmoothCvWork &w, int cur, int F, double sigma_rot, double sigma_rot0, double sigma_trans0, const double *fc,
                               const double *lc, const double *l2, double *terms, double *rec, hipStream_t st);

// live tracker (live_kernels.hip): one frame per push, the whole LM of the window in ONE launch of one workgroup
constexpr int LIVE_MAX_W = 16;            // window frames (AAR_TRACKER_MAX_LAG + 1)
constexpr int LIVE_HDR_BYTES = 64;        // a ring slot starts with the frame's header: pose_init [6] | 2 idle doubles
constexpr int LIVE_REC_BYTES = 48;        // ... followed by its records: ObsIdx (16 bytes) | eight corner coordinates (32 bytes)
constexpr int LIVE_RES_DOUBLES = 24;      // the result record: iterations, stop code, rejected tries, initial / final / data / prior cost, mu,
                                          // the newest pose [8..13], the oldest window pose [14..19], tries, 0
constexpr int LIVE_INFO_DOUBLES = 16;     // the start record of k_live_init, right behind the result record: voted, candidates, winner, vote cost,
                                          // start source, E_f at the prediction, E_f at the vote, 0, the start pose [8..13], 0, 0
// ... and, on a push of raw detections, by one int per record behind the LAST record: the order of the vote's candidates (live_init_kernels.hip)
inline size_t live_slot_bytes(int max_obs) {
    return (LIVE_HDR_BYTES + (size_t)(LIVE_REC_BYTES + sizeof(int32_t)) * (size_t)max_obs + 15) / 16 * 16;
}
struct LiveArgs {
    const double *ent, *Kmat;             // [A][ENT_STRIDE] rows of the fixed cameras and markers, [C][9]
    const char *ring;                     // [lag + 1] slots of slot_bytes
    size_t slot_bytes;
    double *zslot;                        // [lag + 1][6] pose of the frame in each ring slot
    double *anchor;                       // [6] the frame that left the window last
    double *Ef, *Pe;                      // [LIVE_MAX_W] by window position: data cost, cost of the pair that ENDS at the frame (position 0: the anchor pair)
    double *res;                          // [LIVE_RES_DOUBLES]
    float huber; double h;
    int max_iters; double min_error, min_step_error_diff, min_average_step_error_diff, tau;
    int W, slots, first_slot;             // window frames, ring slots (lag + 1), slot of the oldest window frame (the others follow, modulo slots)
    int has_anchor, smooth, has_init;     // has_init: the new frame starts from its header's pose, else from the previous frame's estimate
    double rows;                          // 8 detections of the window + 6 pairs
    int cnt[LIVE_MAX_W];                  // detections by window position
    double lam[LIVE_MAX_W][2];            // by window position: 1 / (sigma_rot^2 dt), 1 / (sigma_trans^2 dt) of the pair that ends there
    // DESIGN.md section 19; marginal = covariance = 0 (and anchor_pair = has_anchor) = the kernel of section 17
    int anchor_pair;                      // the first window frame carries the anchor pair: has_anchor, unless the anchor is marginalised
    int marginal, has_marginal;           // marginalised anchor: no anchor pair; has_marginal: the prior in unc sits on the first window frame
    int covariance;                       // the blocks of H^-1 at the final point
    double *unc;                          // [LIVE_UNC_HDR + 36 LIVE_MAX_W] the uncertainty record (read: the prior; written: the next one)
};
// the uncertainty record, behind the start record: cov_valid, the marginal is valid, it was dropped in this push, 0 | Lambda_m [36] | m [6] | 0 0
// | Sigma_f [36] by window position
constexpr int LIVE_UNC_VALID = 0, LIVE_UNC_HAS = 1, LIVE_UNC_DROP = 2, LIVE_UNC_LM = 4, LIVE_UNC_M = 40, LIVE_UNC_HDR = 48;
constexpr int LIVE_UNC_DOUBLES = LIVE_UNC_HDR + 36 * LIVE_MAX_W;
// a pivot of Lambda' below this fraction of the pair's own J_b^T L J_b diagonal counts as non-positive: what is left of an empty chain is
// rounding noise of either sign around an exact 0
constexpr double LIVE_MARGINAL_PIVOT_REL = 1e-10;
void launch_live_push(const LiveArgs &a, hipStream_t st);   // ONE launch; the tail instance when marginal or covariance is set
// constant-velocity motion model: the same push with an expected motion on every pair -- its own kernel instances
constexpr int LIVE_MOT_DOUBLES = 8;       // the motion record: the pose of the frame before the newest at the final point [0..5], 0 0
struct LiveMotionArgs {
    LiveArgs a;                           // res .. unc lie in the motion tracker's own block, behind the motion record
    double rel[LIVE_MAX_W][6];            // by window position: (rvec, t) expected of the pair that ends there (position 0: the anchor pair's)
    double *mot;                          // [LIVE_MOT_DOUBLES]
};
void launch_live_push_motion(const LiveMotionArgs &a, hipStream_t st);   // ONE launch, as launch_live_push

// tracker bank: B independent live trackers advance in lockstep, workgroup b of k_live_push_bank runs member b's push.
// The ring is [slot][member]: the slots one push fills are contiguous (ONE copy), member b's ring is ring + b slot_bytes with stride B slot_bytes.
// What differs by member and push rides in the slot header's two idle doubles: [6] the frame's detection count, [7] its header holds a start pose.
constexpr int LIVE_HDR_CNT = 6, LIVE_HDR_INIT = 7;
struct LiveMember {                       // one row of the member table, written once at create
    const double *ent, *Kmat;             // the member's solution
    double h;
    const char *ring;                     // bank ring + b slot_bytes
    double *zslot, *anchor, *Ef, *Pe;     // the member's state (as LiveArgs)
    double *res, *unc;                    // the member's records in the bank's output block
};
struct LiveBankArgs {
    LiveArgs sh;                          // what all members share: LM parameters, huber, W, slots, first_slot, has_anchor, smooth, lam, anchor_pair,
                                          // marginal, covariance; slot_bytes = the ring's slot stride B slot_bytes.  The rest is the member's: unused
    const LiveMember *tab;                // [B]
    int raw;                              // the push is of raw detections: k_live_init_bank has written every header's start pose
    int fresh;                            // the first push since creation / reset: no marginal prior whatever the device still holds
};
void launch_live_push_bank(const LiveBankArgs &a, int B, hipStream_t st);   // ONE launch of B workgroups
// the gated single tracker with the motion model: launch_live_push_bank on its one-row table with the expected motions
struct LiveMemberMotionArgs {
    LiveBankArgs ba;
    double rel[LIVE_MAX_W][6];            // as LiveMotionArgs
    double *mot;
};
void launch_live_push_member_motion(const LiveMemberMotionArgs &a, hipStream_t st);   // ONE launch of one workgroup
// the bank with the motion model: every ring slot is the members' slots followed by their expected motions, [B][6] doubles at rel_off (the
// motion of the pair that ENDS at the slot's frame); sh.slot_bytes is the stride of that whole group
struct LiveBankMotionArgs {
    LiveBankArgs ba;
    const char *ring;                     // the bank's ring
    size_t rel_off;                       // B member slots
    double *mot;                          // [B][LIVE_MOT_DOUBLES]
};
void launch_live_push_bank_motion(const LiveBankMotionArgs &a, int B, hipStream_t st);   // ONE launch of B workgroups

// the start of a frame pushed as raw detections (live_init_kernels.hip): undistortion, IPPE, the object pose candidates and
// their vote in ONE launch of one workgroup, on the slot the frame was just copied into
constexpr int LIVE_START_VOTE = 1, LIVE_START_BEST = 2;   // AAR_TRACKER_START_*
struct LiveInitArgs {
    char *slot;                           // header | n_det records (raw corners in, P = K corners out) | n_det ints: detections in candidate order
    int n_det;
    const void *cams;                     // [C] CamTab (ippe_vote.hpp): K and twelve distortion coefficients by camera index
    const double *Tcr, *Tmr;              // [C][12], [M][12] to-root transforms of the solution (the identity for the roots)
    int C;                                // a record's marker entity is C + marker index
    float hf; double h;                   // half marker side: float for IPPE, double for the vote
    double threshold;                     // second IPPE solution kept when (double)e2 / (double)e1 < threshold
    int do_vote, policy, has_init, has_prev;
    const double *zprev;                  // [6] the previous frame's estimate (has_prev)
    const double *ent, *Kmat; float huber; double h_track;   // k_live_push's model, for E_f at the two starts (LIVE_START_BEST)
    double *poses; int *has2;             // workspace: [2 max_obs][12], [max_obs]
    double *Tc, *BJ, *cost; int *fin;     //            [2 max_obs][12], [2 max_obs][24], [2 max_obs], [2 max_obs]
    double *info;                         // [LIVE_INFO_DOUBLES]
};
void launch_live_init(const LiveInitArgs &a, hipStream_t st);   // ONE launch
// the doubles of one k_live_init workspace (poses | Tc | BJ | cost, then has2 | fin as ints), and its carving
inline size_t live_init_work_doubles(size_t max_obs) { return 98 * max_obs + (3 * max_obs * sizeof(int) + sizeof(double) - 1) / sizeof(double); }
__host__ __device__ inline void live_init_work_carve(LiveInitArgs &a, double *work, size_t max_obs) {
    a.poses = work; a.Tc = a.poses + 24 * max_obs; a.BJ = a.Tc + 24 * max_obs; a.cost = a.BJ + 48 * max_obs;
    a.has2 = reinterpret_cast<int *>(a.cost + 2 * max_obs); a.fin = a.has2 + max_obs;
}
// the bank's start: workgroup b does k_live_init's work on member b's new slot, in its own workspace slice
struct LiveInitMember {                   // one row of the table, written at aar_tracker_bank_enable_detections
    const void *cams; const double *Tcr, *Tmr;
    int C, policy, min_detections;
    float hf; double h, threshold;
    const double *ent, *Kmat; double h_track;
    const double *zslot;                  // the member's poses by ring slot
    double *work;                         // live_init_work_doubles(max_obs) of its own
    double *info;
};
struct LiveInitBankArgs {
    const LiveInitMember *tab;            // [B]
    char *slot0;                          // the new slot of member 0; member b's follows at b slot_bytes
    size_t slot_bytes, max_obs;
    int has_prev, prev_slot;              // a previous frame exists, its ring slot
    float huber;
    int pred_in_header;                   // motion model: a member without a start pose finds its prediction in its slot header, not in zslot
};
void launch_live_init_bank(const LiveInitBankArgs &a, int B, hipStream_t st);   // ONE launch of B workgroups

// the gate of a pushed frame (live_gate_kernels.hip): aar_outlier_rule on the NEW frame at the pose the push starts from,
// the slot's records compacted in place and the kept count written into the header's LIVE_HDR_CNT -- ONE launch between start and refinement
constexpr int LIVE_GATE_MAX_OBS = 4096;   // the exact median sorts the frame's errors in one workgroup's LDS
constexpr int LIVE_GATE_DOUBLES = 8;      // the gate record: gated, n_in, n_kept, n_nonfinite, median, max, threshold, 0
struct LiveGateParams {
    double k_median, min_px;
    int min_detections;
};
struct LiveGateArgs {
    char *slot;                           // header | n records
    int n, has_init;                      // has_init: the start pose is the header's (pose_init, or k_live_init's choice), else zprev
    const double *zprev;                  // [6] the previous frame's estimate
    const double *ent, *Kmat; double h;   // k_live_push's model
    LiveGateParams g;
    double *rec;                          // [LIVE_GATE_DOUBLES]
    double *det_err; uint8_t *keep;       // [max_obs] each, in the caller's order
};
void launch_live_gate(const LiveGateArgs &a, hipStream_t st);   // ONE launch
struct LiveGateMember {                   // one row of the table, written at aar_tracker_gate_bank_enable
    const double *ent, *Kmat; double h;
    const double *zslot;                  // the member's poses by ring slot
    double *rec, *det_err; uint8_t *keep;
};
struct LiveGateBankArgs {
    const LiveGateMember *tab;            // [B]
    char *slot0;                          // the new slot of member 0; member b's follows at b slot_bytes
    size_t slot_bytes;
    int raw, prev_slot;                   // raw: k_live_init_bank wrote every header's start pose; the previous frame's ring slot
    LiveGateParams g;
};
void launch_live_gate_bank(const LiveGateBankArgs &a, int B, hipStream_t st);   // ONE launch of B workgroups

// covariance (cov_kernels.hip): S (stride n_pad) -> S2 (stride n2 >= n_pad, zero beyond n_pad), rows with rowmask set -> identity
void launch_cov_stage(const double *S, int n_pad, double *S2, int n2, const int32_t *rowmask, hipStream_t st);
// the LDL^T factor launch_chol left for S2 (nT2 tiles, fused_m = the panel rule it ran with) -> Sinv = S^-1, lower 32 x 32 tiles of the first
// n_pad rows; Lc, X: [n_pad][n_pad] scratch, Dinv: [n_pad] = 1 / D
void launch_cov_inverse(const double *S2, const double *Dfac, const double *Lp, int n_pad, int n2, int nT2, int fused_m, double *Lc, double *Dinv,
                        double *X, double *Sinv, hipStream_t st);
// out[a][36] = the 6x6 diagonal block of entity a in Sinv
void launch_cov_diag_blocks(const double *Sinv, int n_pad, int A, double *out, hipStream_t st);
// out[f][36] = (J^T J)^-1 block of local frame f from Vinv of block set `which` (mu = 0), its W blocks and Sinv
void launch_cov_frames(const DeviceProblem &P, int which, const double *Sinv, const int32_t *rowmask, double *out, hipStream_t st);

// predicted corners with covariance, detection leverages (predict_kernels.hip).  The row mask of the covariance
// chain with a second value: a row without an unknown is PREDICT_CONST where the parameter is a constant (root, non-optimised group,
// fixed by the caller, padding: ZERO covariance) and PREDICT_UNSEEN where it has a z column that nothing determines (covariance undefined).
// k_cov_stage and k_cov_frames only ask whether a row is masked at all.
constexpr int PREDICT_LIVE = 0, PREDICT_CONST = 1, PREDICT_UNSEEN = 2;
struct PredictArgs {
    const double *ent, *K;                // entity rows of the point (launch_unpack), camera matrices K[kstride * camera + i]
    int kstride, C, A;                    // cameras, shared entities (frame f's row is A + f)
    double h;
    int64_t n;                            // queries
    const int32_t *q_cam, *q_marker, *q_frame;   // explicit queries: camera, marker and frame INDEX (modes 0, 1)
    const ObsIdx *obs;                    // ... or the problem's ordering A (mode 2)
    const int32_t *fslot_start, *fslot_ent, *rowmask;   // rowmask [n_pad]: PREDICT_*
    int frames_opt, n_pad;                // 0: the frames are constants, gain / frame_cov are not touched
    const double *gain, *Sinv, *frame_cov;   // launch_predict_gains' [total_slots][36], S^-1 (lower triangle), launch_cov_frames' [F][36]
    double *uv, *cov;                     // [n][8], [n][64] (modes 0, 1; cov mode 0 only)
    uint8_t *status;                      // [n] bit 0: a corner at non-positive depth, bit 1: covariance undefined
    double *lev, *row_lev;                // [n], [n][8] or NULL (mode 2): trace and diagonal of C
    // modes 3, 4 (leave-one-out residuals, gate of candidate detections: DESIGN.md section 37).  r = observed - u, A = I - C (3) / I + C (4)
    const float *obs_uv;                  // observed corners [n][8]: ordering A's (mode 3), the caller's (mode 4)
    double *loo_w, *loo_q, *loo_k, *loo_margin;   // [n][8] w = A^-1 r (mode 4: r itself), [n] r^T w, [n] w^T C w (mode 3), [n] smallest pivot
    double *loo_F, *loo_cook;             // [n] (mode 3)
    uint8_t *loo_keep;                    // [n] (mode 3)
    double sum_sq, cook_den, f_max;       // (mode 3) the chain's sum r^2, num_live_vars * sigma2, the rule's bound (0: no rule)
    int64_t dof;                          // (mode 3) nu = num_residuals - num_vars
};
// A pivot L_kk^2 of I - C_i at or below this (or not finite) makes the detection UNDETERMINED: nothing but itself determines some
// direction of its corners, and a fit without it does not exist.  A stated choice: well above the absolute error measured for an
// entry of C (<= 4e-8 on the test sets), far below any 1 - lambda at which a deleted fit still means something.
constexpr double PREDICT_LOO_MIN_PIVOT = 1e-6;
constexpr int PREDICT_UNDETERMINED = 4;   // status bit 2 (AAR_PREDICT_UNDETERMINED)
// gain[s][36] = V_f^-1 W_s^T for every slot s (frame f's slots at fslot_start[f]), masked rows' columns zero: needs Vinv at mu = 0 and the fp64 W
void launch_predict_gains(const DeviceProblem &P, int which, const int32_t *rowmask, double *gain, hipStream_t st);
// mode 0: uv | cov | status of explicit queries, 1: uv | status alone (nothing of the chain is read), 2: lev | row_lev | status of the
// problem's own detections in reference order.  One launch, one wavefront per query
void launch_predict_corners(const PredictArgs &a, int mode, hipStream_t st);

// the same quantities on a smoothed track (smooth_predict_kernels.hip): Sigma is one 6 x 6 block of the smoother's H^-1,
// G the frame Jacobian alone.  The problem's detections (modes 2, 3) read pose[frame] and block[frame]: z [F][6] and SmoothSel.fc.  Explicit
// queries (modes 0, 1, 4) read pose[q] and block[q]: the poses and blocks the query chain left for the queries' times.  Mode 1 reads no block
struct SmoothCornersArgs {
    const double *ent, *K;                // entity rows of the cameras and markers (launch_unpack), camera matrices K[kstride * camera + i]
    int kstride, C;
    double h;
    int64_t n;                            // queries
    const ObsIdx *obs;                    // ordering A (modes 2, 3) ...
    const int32_t *q_cam, *q_marker;      // ... or camera and marker INDEX per query (modes 0, 1, 4)
    const double *pose, *block;           // [.][6], [.][36]
    double *uv, *cov;                     // [n][8], [n][64] (modes 0, 1; cov mode 0 only)
    uint8_t *status;                      // [n] bit 0: a corner at non-positive depth, bit 2 (modes 3, 4): PREDICT_UNDETERMINED
    double *lev, *row_lev;                // [n], [n][8] or NULL (mode 2; lev also mode 3)
    const float *obs_uv;                  // observed corners [n][8]: ordering A's (mode 3), the caller's (mode 4)
    double *loo_w, *loo_q, *loo_margin;   // [n][8] w = A^-1 r (mode 4: r itself), [n] r^T w, [n] smallest pivot
    double *loo_F, *loo_cook;             // [n] (mode 3)
    uint8_t *loo_keep;                    // [n] (mode 3)
    const double *res;                    // (mode 3) the chain's record ON THE DEVICE: data cost, prior cost
    double f_max, num_vars;               // (mode 3) the rule's bound (0: no rule), 6 F
    int64_t dof;                          // (mode 3) nu = num_residuals - num_vars
};
// one launch, eight lanes per query
void launch_smooth_corners(const SmoothCornersArgs &a, int mode, hipStream_t st);

// residual report (resid_kernels.hip).  The select's state: the key bits [pshift, 63) picked so far, the rank still
// wanted inside that bucket, done (prefix = the key), single (one key left in the bucket: the next pass fetches it), t = the threshold
constexpr int RR_DIGIT_BITS = 11, RR_BINS = 1 << RR_DIGIT_BITS, RR_PASSES = 6;   // 63 key bits = 5 digits of 11 + one of 8
struct RRSel {
    unsigned long long prefix, rank;
    double t;
    int pshift, done, single, pad;
};
// device buffers of the report (allocated by the first call of a problem): per observation of ordering A err, ss (its sum r^2), keep;
// [F][4] frame stats; ordering B as runs of (camera, marker): perm (B -> A), run_start [R+1]; cam_run_start [C+1] (runs of a camera are
// contiguous), mk_run_start [M+1] / mk_runs [R] (the runs of a marker, camera-ascending); rstat [R][5], rmax [R]; esum [5 (C+M) + 1],
// emax [C+M] (k_rr_entities); hist: [RR_BINS] counts | 2 halves of a found key | frames-emptied counter; hd: hist as doubles
struct RRWork {
    double *err = nullptr, *ss = nullptr, *fstat = nullptr, *rstat = nullptr, *esum = nullptr, *emax = nullptr, *hd = nullptr;
    uint8_t *keep = nullptr;
    int32_t *perm = nullptr, *run_start = nullptr, *cam_run_start = nullptr, *mk_run_start = nullptr, *mk_runs = nullptr;
    unsigned long long *rmax = nullptr;
    uint32_t *hist = nullptr;
    RRSel *sel = nullptr;
    int R = 0;
};
constexpr int RR_HIST_WORDS = RR_BINS + 3;
// e_d, ss, frame stats [0..2] and the first digit's histogram at z[which] (ent[which] must hold its rows); starts the select for `rank`
void launch_rr_errors(const DeviceProblem &P, int which, const RRWork &w, unsigned long long rank, hipStream_t st);
void launch_rr_select_pass(const DeviceProblem &P, const RRWork &w, hipStream_t st);   // the next digit's histogram
void launch_rr_to_double(const RRWork &w, hipStream_t st);                               // hist -> hd (the all-reduce payload)
void launch_rr_pick(const RRWork &w, bool reduced, hipStream_t st);                      // reduced: read hd instead of hist
// threshold, keep flags, rejected per frame, the run and entity sums
void launch_rr_stats(const DeviceProblem &P, const RRWork &w, int has_rule, double k_median, double min_px, hipStream_t st);

// The error flags of a rank (bits 0..3) as one double that survives a SUM all-reduce over up to 4095 ranks: bit b set on k ranks adds k 4096^b.
// Every rank decodes the same value, so every rank takes the same branch (a rank that failed alone would otherwise leave the
// others waiting in their next collective).
__device__ __forceinline__ double encode_flags(int f) {
    return (double)(f & 1) + 4096.0 * (double)((f >> 1) & 1) + 16777216.0 * (double)((f >> 2) & 1) + 68719476736.0 * (double)((f >> 3) & 1);
}
__device__ __forceinline__ int decode_flags(double v) {
    const long long q = (long long)v;
    return ((q % 4096) ? 1 : 0) | (((q / 4096) % 4096) ? 2 : 0) | (((q / 16777216) % 4096) ? 4 : 0) | ((q / 68719476736LL) ? 8 : 0);
}

// flags_reduced: the flags come from scal[3] (all ranks' flags, summed by the all-reduce) instead of this rank's flag words
__device__ __forceinline__ void publish_host(const double *__restrict__ scal, const int32_t *__restrict__ flags,
                                             double *__restrict__ host, unsigned long long seq, int flags_reduced = 0) {
#pragma unroll
    for (int i = 0; i < 8; i++) host[i] = scal[i];
    reinterpret_cast<long long *>(host)[8] = flags_reduced ? (long long)decode_flags(scal[3]) : (long long)(flags[0] | flags[1] | flags[2] | flags[3]);
    __threadfence_system();
    __hip_atomic_store(reinterpret_cast<unsigned long long *>(host) + 9, seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
}


}  // namespace aar
