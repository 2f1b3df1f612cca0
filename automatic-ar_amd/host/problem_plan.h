// The index tables of a problem (orderings A and B, slot lists, the Schur work lists, the deterministic mode's reduction records,
// the MFMA kernel's dense numbering, the PCG work items, the pair priors' element lists): pure host arithmetic on the observation
// list, built here without a device, an environment variable or a HIP header.  problem_create (csrc/ba_capi.hip) resolves the knobs,
// calls the two stages around its choice of the solver and uploads what they return; every kernel trusts these tables.
// Fields are named as the DeviceProblem fields they fill (csrc/kernels.h).
#pragma once
#include <cstdint>
#include <optional>
#include <vector>

#include "internal.h"
#include "plan_types.h"

namespace aar {

// DeviceProblem::pair_rec (an int4 on the device): {frame, W block, first W block of the frame, 0}
struct PairRec {
    int32_t frame, slot, frame_slot0, pad;
};

// Frame stage: what the choice of the solver needs (max_kf, total_slots) and everything that is per frame
struct FramePlan {
    int A = 0, F = 0;          // shared entities (C + M, + C with intrinsics), local frames
    int64_t N = 0;             // local observations
    std::vector<ObsIdx> a_idx;   // ordering A = reference order
    std::vector<float> a_uv;
    std::vector<int32_t> frame_obs_start, frame_stride, fslot_start, fslot_ent;
    int max_kf = 0, total_slots = 0;
    int status = 0;            // AAR_OK, or AAR_ERR_UNSUPPORTED (message set): a frame of this rank touches too many entities
};
// per_frame: observations of every frame of the whole data set; [f_begin, f_end) this rank's frames, o_begin its first observation
FramePlan plan_frames(const aar_problem_desc &d, const PoseLayout &L, const std::vector<int64_t> &per_frame, int f_begin, int f_end, int64_t o_begin);

// Ordering B: the stable sort of ordering A by (camera, marker, frame) and its (camera, marker) runs
struct OrderingB {
    std::vector<int32_t> perm;        // [N] position in B -> position in A
    std::vector<int32_t> run_start;   // [R + 1] into ordering B
};
OrderingB plan_ordering_b(const ObsIdx *a_idx, int64_t N);

// The resolved knobs of the table stage; an empty optional = the environment variable of that name is not set
struct PlanKnobs {
    bool deterministic = false, schur_mfma = false, use_pcg = false;
    int n_cus = 256;
    std::optional<int> passb_chunk, schur_item, schur_window, schur_xcd, schur_split;   // AAR_PASSB_CHUNK, AAR_SCHUR_ITEM, AAR_SCHUR_WINDOW, AAR_SCHUR_XCD, AAR_SCHUR_SPLIT
    std::optional<long long> pcg_chunk;                                                 // AAR_PCG_CHUNK
};

struct TablePlan {
    std::vector<ObsIdx> b_idx;   // ordering B
    std::vector<float> b_uv;
    std::vector<int32_t> chunk_start;
    int n_chunks = 0;
    std::vector<int32_t> ent_fixed, up_start, up_ent;
    std::vector<int32_t> sw_ent, sw_begin, sw_end;
    std::vector<PairRec> pair_rec;
    int n_swork = 0;
    // deterministic mode
    std::vector<int64_t> sp_off;
    std::vector<int32_t> se_start, se_items, pbr_start, pbr_chunk, pbr_kind, pbr_a, pbr_b;
    int64_t sp_total = 0;      // doubles of DeviceProblem::sp_part
    int n_pbr = 0, pb_stride = 0;
    // MFMA Schur kernel
    std::vector<int32_t> sm_ga, sm_gb, sm_fb, sm_fe, slot_frame, slot_dense, dense_ent, sm_frames;
    int Ad = 0, n_smwork = 0;
    // solver pcg
    std::vector<int32_t> pcg_it_ent, pcg_it_begin, pcg_it_end, pcg_ent_item_start;
    int pcg_n_items = 0;
    // pair priors (empty without any)
    std::vector<int32_t> pair_ends, pair_el_ent, pair_el_start, pair_el_item;
    int n_pair_el = 0, n_pair_items = 0;
};
// cons: validated and not empty, or NULL
TablePlan plan_tables(const PoseLayout &L, const FramePlan &fp, const aar_problem_constraints *cons, const PlanKnobs &knobs);

// [C + M] entities the caller fixed that would be free otherwise
std::vector<int32_t> plan_held_entities(const PoseLayout &L, const aar_problem_constraints *cons);

}  // namespace aar
