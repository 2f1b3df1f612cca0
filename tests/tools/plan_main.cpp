// Builds the index tables of one case of tests/plan_cases.py with the planner (host/problem_plan.cpp) and writes them to a file, in the
// record format of plan_cases.read_dump.  Host code only: g++ over this file, host/problem_plan.cpp, host/synth.cpp and host/dataset.cpp.
//     plan_main OUT key=value ...      (the keys: plan_cases.plan_main_args)
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../automatic-ar_amd/host/problem_plan.h"

using namespace aar;

static FILE *g_out = nullptr;

template <class T>
static void dump(const char *name, const std::vector<T> &vec) {
    char nm[32] = {0};
    strncpy(nm, name, 31);
    const int32_t es = (int32_t)sizeof(T);
    const int64_t cnt = (int64_t)vec.size();
    fwrite(nm, 1, 32, g_out); fwrite(&es, 4, 1, g_out); fwrite(&cnt, 8, 1, g_out);
    if (cnt) fwrite(vec.data(), es, cnt, g_out);
}
static void dump_count(const char *name, int64_t v) { dump(name, std::vector<int64_t>{v}); }

int main(int argc, char **argv) {
    if (argc < 2) { fputs("usage: plan_main OUT key=value ...\n", stderr); return 2; }
    int frames = 40, cams = 0, markers = 0, drop_frame = -1, intrinsics = 0, world = 1, rank = 0;
    double min_view_cos = -1.0;
    PlanKnobs knobs;
    std::vector<int32_t> fixed_cams, fixed_markers;
    std::vector<aar_pair_prior> pairs;
    for (int i = 2; i < argc; i++) {
        const char *eq = strchr(argv[i], '=');
        if (!eq) { fprintf(stderr, "bad argument %s\n", argv[i]); return 2; }
        const std::string k(argv[i], eq - argv[i]);
        const char *v = eq + 1;
        if (k == "frames") frames = atoi(v);
        else if (k == "cams") cams = atoi(v);
        else if (k == "markers") markers = atoi(v);
        else if (k == "min_view_cos") min_view_cos = atof(v);
        else if (k == "drop_frame") drop_frame = atoi(v);
        else if (k == "intrinsics") intrinsics = atoi(v);
        else if (k == "deterministic") knobs.deterministic = atoi(v) != 0;
        else if (k == "use_pcg") knobs.use_pcg = atoi(v) != 0;
        else if (k == "schur_mfma") knobs.schur_mfma = atoi(v) != 0;
        else if (k == "n_cus") knobs.n_cus = atoi(v);
        else if (k == "world") world = atoi(v);
        else if (k == "rank") rank = atoi(v);
        else if (k == "passb_chunk") knobs.passb_chunk = atoi(v);
        else if (k == "schur_item") knobs.schur_item = atoi(v);
        else if (k == "schur_window") knobs.schur_window = atoi(v);
        else if (k == "schur_xcd") knobs.schur_xcd = atoi(v);
        else if (k == "schur_split") knobs.schur_split = atoi(v);
        else if (k == "pcg_chunk") knobs.pcg_chunk = atoll(v);
        else if (k == "fixed_cam") fixed_cams.push_back(atoi(v));
        else if (k == "fixed_marker") fixed_markers.push_back(atoi(v));
        else if (k == "pair") {   // c:a:b | m:a:b
            aar_pair_prior q;
            memset(&q, 0, sizeof q);
            int a = 0, b = 0;
            if (sscanf(v + 1, ":%d:%d", &a, &b) != 2) { fprintf(stderr, "bad pair %s\n", v); return 2; }
            q.kind = v[0] == 'c' ? AAR_PRIOR_CAMERA : AAR_PRIOR_MARKER; q.index_a = a; q.index_b = b;
            for (int d = 0; d < 6; d++) q.info[7 * d] = 1.0;
            pairs.push_back(q);
        } else { fprintf(stderr, "unknown key %s\n", k.c_str()); return 2; }
    }
    aar_synth_desc sd;
    aar_synth_default(&sd, 3);
    sd.num_frames = frames;
    if (cams > 0) sd.num_cams = cams;
    if (markers > 0) sd.num_markers = markers;
    if (min_view_cos >= 0) sd.min_view_cos = min_view_cos;
    aar_dataset *ds = nullptr;
    if (aar_synth_generate(&sd, &ds)) { fprintf(stderr, "%s\n", aar_last_error()); return 1; }
    if (drop_frame >= 0) {
        std::vector<uint8_t> keep(ds->num_obs);
        for (int64_t o = 0; o < ds->num_obs; o++) keep[o] = ds->obs_frame[o] != drop_frame;
        aar_dataset *cut = nullptr;
        if (aar_dataset_select_observations(ds, keep.data(), &cut)) { fprintf(stderr, "%s\n", aar_last_error()); return 1; }
        aar_dataset_free(ds);
        ds = cut;
    }
    aar_problem_desc d;
    aar_problem_desc_from_dataset(ds, &d);
    d.optimize_cam_intrinsics = intrinsics;
    aar_problem_constraints cons;
    memset(&cons, 0, sizeof cons);
    cons.struct_size = (uint32_t)sizeof cons;
    cons.n_fixed_cams = (int32_t)fixed_cams.size(); cons.fixed_cams = fixed_cams.data();
    cons.n_fixed_markers = (int32_t)fixed_markers.size(); cons.fixed_markers = fixed_markers.data();
    cons.n_pair_priors = (int32_t)pairs.size(); cons.pair_priors = pairs.data();
    const bool with_cons = !fixed_cams.empty() || !fixed_markers.empty() || !pairs.empty();

    PoseLayout L;
    L.C = d.num_cams; L.M = d.num_markers; L.F = d.num_frames; L.rc = d.root_cam; L.rm = d.root_marker;
    L.oc = d.optimize_cam_poses != 0; L.om = d.optimize_marker_poses != 0; L.of = d.optimize_object_poses != 0; L.oi = intrinsics != 0;
    std::vector<int64_t> per_frame(d.num_frames, 0);
    for (int64_t o = 0; o < d.num_obs; o++) per_frame[d.obs_frame[o]]++;
    std::vector<int32_t> begin(world + 1, 0);
    if (aar_plan_shards(d.num_frames, per_frame.data(), world, begin.data())) { fprintf(stderr, "%s\n", aar_last_error()); return 1; }
    int64_t o_begin = 0;
    for (int f = 0; f < begin[rank]; f++) o_begin += per_frame[f];

    FramePlan fp = plan_frames(d, L, per_frame, begin[rank], begin[rank + 1], o_begin);
    if (fp.status) { fprintf(stderr, "%s\n", aar_last_error()); return 1; }
    const TablePlan T = plan_tables(L, fp, with_cons ? &cons : nullptr, knobs);

    g_out = fopen(argv[1], "wb");
    if (!g_out) { perror(argv[1]); return 1; }
    dump("a_idx", fp.a_idx); dump("frame_obs_start", fp.frame_obs_start); dump("frame_stride", fp.frame_stride);
    dump("fslot_start", fp.fslot_start); dump("fslot_ent", fp.fslot_ent); dump("b_idx", T.b_idx);
    dump("chunk_start", T.chunk_start); dump("ent_fixed", T.ent_fixed); dump("up_start", T.up_start); dump("up_ent", T.up_ent);
    dump("sw_ent", T.sw_ent); dump("sw_begin", T.sw_begin); dump("sw_end", T.sw_end); dump("pair_rec", T.pair_rec);
    if (knobs.use_pcg) { dump("pcg_it_ent", T.pcg_it_ent); dump("pcg_it_begin", T.pcg_it_begin); dump("pcg_it_end", T.pcg_it_end); dump("pcg_ent_item_start", T.pcg_ent_item_start); }
    if (knobs.deterministic) {
        dump("sp_off", T.sp_off); dump("se_start", T.se_start); dump("se_items", T.se_items); dump("pbr_start", T.pbr_start); dump("pbr_chunk", T.pbr_chunk);
        dump("pbr_kind", T.pbr_kind); dump("pbr_a", T.pbr_a); dump("pbr_b", T.pbr_b);
    }
    if (T.n_smwork) {
        dump("sm_ga", T.sm_ga); dump("sm_gb", T.sm_gb); dump("sm_fb", T.sm_fb); dump("sm_fe", T.sm_fe); dump("slot_dense", T.slot_dense); dump("slot_frame", T.slot_frame);
        dump("dense_ent", T.dense_ent); dump("sm_frames", T.sm_frames);
    }
    if (!pairs.empty()) { dump("pair_ends", T.pair_ends); dump("pair_el_ent", T.pair_el_ent); dump("pair_el_start", T.pair_el_start); dump("pair_el_item", T.pair_el_item); }
    dump_count("n_chunks", T.n_chunks); dump_count("n_swork", T.n_swork); dump_count("n_smwork", T.n_smwork); dump_count("Ad", T.Ad); dump_count("max_kf", fp.max_kf);
    dump_count("total_slots", fp.total_slots); dump_count("n_pbr", T.n_pbr); dump_count("pb_stride", T.pb_stride); dump_count("pcg_n_items", T.pcg_n_items); dump_count("sp_total", T.sp_total);
    dump_count("n_pair_el", T.n_pair_el); dump_count("n_pair_items", T.n_pair_items);
    // what the golden file does not hold: the test checks them through the permutation
    dump("a_uv_bits", std::vector<int32_t>((const int32_t *)fp.a_uv.data(), (const int32_t *)fp.a_uv.data() + fp.a_uv.size()));
    dump("b_uv_bits", std::vector<int32_t>((const int32_t *)T.b_uv.data(), (const int32_t *)T.b_uv.data() + T.b_uv.size()));
    fclose(g_out);
    aar_dataset_free(ds);
    return 0;
}
