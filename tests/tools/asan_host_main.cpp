#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>
#include "../../include/aar.h"
#include "../../automatic-ar_amd/host/init_device.h"
#include "../../automatic-ar_amd/host/problem_plan.h"
// device entry points stubbed: this binary exercises the HOST code under ASan/UBSan only
namespace aar {
int initdev_create(int32_t, InitDevice **) { return set_error(AAR_ERR_NO_DEVICE, "stub"); }
void initdev_destroy(InitDevice *) {}
int initdev_ippe(InitDevice *, const aar_cam_model *, int32_t, float, int64_t, const float *, const int32_t *, float *, float *, float *) { return -2; }
int initdev_pair_vote(InitDevice *, int, int64_t, const int32_t *, const int32_t *, int64_t, const int64_t *, double, int64_t *, double *, double *) { return -2; }
int initdev_object_vote(InitDevice *, int64_t, const int32_t *, const int32_t *, const int32_t *, int32_t, const double *, int32_t, const double *, int64_t, const int64_t *, double, int64_t *, double *, double *) { return -2; }
}
extern "C" int aar_undistort_points(const double *, const double *, int32_t, int64_t, const float *, float *, int32_t) { return -2; }
// the problem planner (host/problem_plan.cpp) on one data set: both stages, as problem creation calls them
static void plan(const char *what, const aar_dataset *ds, bool intrinsics, const aar_problem_constraints *cons, const aar::PlanKnobs &knobs) {
    aar_problem_desc d;
    memset(&d, 0, sizeof d);
    const double K1[9] = {500, 0, 320, 0, 500, 240, 0, 0, 1};
    if (ds) aar_problem_desc_from_dataset(ds, &d);
    else { d.num_cams = 2; d.num_markers = 3; d.cam_mats = K1; d.optimize_cam_poses = d.optimize_marker_poses = d.optimize_object_poses = 1; }   // the empty problem: no frame, no observation
    aar::PoseLayout L;
    L.C = d.num_cams; L.M = d.num_markers; L.F = d.num_frames; L.rc = d.root_cam; L.rm = d.root_marker; L.oi = intrinsics;
    std::vector<int64_t> per_frame(d.num_frames, 0);
    for (int64_t o = 0; o < d.num_obs; o++) per_frame[d.obs_frame[o]]++;
    const aar::FramePlan fp = aar::plan_frames(d, L, per_frame, 0, d.num_frames, 0);
    const aar::TablePlan tp = aar::plan_tables(L, fp, cons, knobs);
    printf("plan %s: chunks %d items %d mfma items %d reduction records %d pair elements %d\n", what, tp.n_chunks, tp.n_swork, tp.n_smwork, tp.n_pbr, tp.n_pair_el);
}

int main(int argc, char **argv) {
    // every file of the run lives under the directory given as the only argument (the caller's scratch directory)
    if (argc != 2) { fputs("usage: asan_host_main DIR\n", stderr); return 2; }
    const std::string dir = argv[1];
    auto P = [&](const char *rel) { return dir + rel; };
    aar_synth_desc sd; aar_synth_default(&sd, 3); sd.num_frames = 40;
    aar_dataset *d = nullptr;
    if (aar_synth_generate(&sd, &d)) { puts(aar_last_error()); return 1; }
    if (system(("mkdir -p '" + dir + "/cam_000' '" + dir + "/cam_001'").c_str())) return 1;
    aar_detections_write(P("/aruco.detections").c_str(), d);
    aar_solution_write(P("/i.solution").c_str(), d);
    aar_solution_write_yaml(P("/i.solution.yaml").c_str(), d);
    aar_dataset *d2 = nullptr;
    if (aar_solution_read(P("/i.solution").c_str(), &d2)) { puts(aar_last_error()); return 1; }
    printf("obs %lld %lld\n", (long long)d->num_obs, (long long)d2->num_obs);
    aar_detections *det = nullptr;
    int32_t ss[4] = {2, 5, 10, 12};
    if (aar_detections_read(P("/aruco.detections").c_str(), ss, 4, &det)) { puts(aar_last_error()); return 1; }
    printf("det %lld frames %d cams %d\n", (long long)det->num_det, det->num_frames, det->num_cams);
    // truncated file
    { FILE *f = fopen(P("/aruco.detections").c_str(), "rb"); fseek(f, 0, SEEK_END); long n = ftell(f); fseek(f, 0, SEEK_SET);
      std::vector<char> b(n); fread(b.data(), 1, n, f); fclose(f);
      for (long cut : {0L, 3L, 8L, 9L, 20L, n / 2, n - 1}) { f = fopen(P("/t.det").c_str(), "wb"); fwrite(b.data(), 1, cut, f); fclose(f);
        aar_detections *t = nullptr; int rc = aar_detections_read(P("/t.det").c_str(), nullptr, 0, &t); if (!rc) aar_detections_free(t); } }
    const char *yml = "%YAML:1.0\n---\nimage_width: 640\nimage_height: 480\ncamera_matrix: !!opencv-matrix\n   rows: 3\n   cols: 3\n   dt: d\n   data: [ 500., 0., 320., 0., 500., 240., 0., 0., 1. ]\ndistortion_coefficients: !!opencv-matrix\n   rows: 1\n   cols: 5\n   dt: d\n   data: [ 0.1, 0., 0., 0., 0. ]\n";
    for (const char *p : {"/cam_000/calib.yml", "/cam_001/calib.yml"}) { FILE *f = fopen(P(p).c_str(), "w"); fputs(yml, f); fclose(f); }
    { FILE *f = fopen(P("/cam_001/calib.xml").c_str(), "w"); fputs("<?xml version=\"1.0\"?><opencv_storage><image_width>1</image_width>", f); fclose(f); }   // malformed
    aar_cam_model *cams = nullptr; int32_t nc = 0;
    aar_cam_configs_read(dir.c_str(), &cams, &nc);
    printf("cams %d\n", nc);
    aar_init_params ip; aar_init_default_params(&ip);
    aar_dataset *o = nullptr;
    int rc = aar_initializer_run(det, cams, nc, &ip, &o);   // reaches the device stub: NO_DEVICE
    printf("init rc %d (%s)\n", rc, aar_last_error());
    int32_t begin[9]; std::vector<int64_t> per(d->num_frames, 3);
    aar_plan_shards(d->num_frames, per.data(), 8, begin);
    int32_t *sub = nullptr, nsub = 0; { FILE *f = fopen(P("/subseqs.txt").c_str(), "w"); fputs("1 2\n7 9 x", f); fclose(f); }
    aar_subseqs_read(P("/subseqs.txt").c_str(), &sub, &nsub); printf("subseqs %d\n", nsub); free(sub);
    {   // the index tables: default, deterministic (with intrinsics), the MFMA work list, solver pcg, pair priors, and the empty problem
        aar::PlanKnobs k0, kdet, kmfma, kpcg;
        kdet.deterministic = true; kdet.schur_xcd = 1;
        kmfma.schur_mfma = true; kmfma.schur_split = 4; kmfma.schur_window = 8;
        kpcg.use_pcg = kpcg.schur_mfma = true; kpcg.pcg_chunk = 1; kpcg.passb_chunk = 64;
        plan("default", d, false, nullptr, k0);
        plan("deterministic", d, true, nullptr, kdet);
        plan("mfma", d, false, nullptr, kmfma);
        int32_t fixed_cam = 2, fixed_marker = 3;
        aar_pair_prior pp[3];
        memset(pp, 0, sizeof pp);
        pp[0].kind = AAR_PRIOR_CAMERA; pp[0].index_a = 1; pp[0].index_b = 2 + 1;
        pp[1].kind = AAR_PRIOR_MARKER; pp[1].index_a = 3; pp[1].index_b = 4;
        pp[2].kind = AAR_PRIOR_CAMERA; pp[2].index_a = d->root_cam; pp[2].index_b = 4;
        aar_problem_constraints cons;
        memset(&cons, 0, sizeof cons);
        cons.struct_size = (uint32_t)sizeof cons;
        cons.n_fixed_cams = 1; cons.fixed_cams = &fixed_cam; cons.n_fixed_markers = 1; cons.fixed_markers = &fixed_marker;
        cons.n_pair_priors = 3; cons.pair_priors = pp;
        plan("pair priors", d, false, &cons, k0);
        plan("pcg", d, false, &cons, kpcg);
        plan("empty", nullptr, false, nullptr, k0);
        plan("empty, deterministic", nullptr, true, nullptr, kdet);
        plan("empty, mfma", nullptr, false, nullptr, kmfma);
    }
    free(cams); aar_detections_free(det); aar_dataset_free(d); aar_dataset_free(d2);
    return 0;
}
