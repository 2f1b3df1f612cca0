// Test driver (not part of the product): MultiCamMapper::track(), track_smooth() under the given motion model and then the per-detection
// layer of the smoothed track BY ID -- track_smooth_detection_leverage, track_smooth_detection_loo, track_smooth_predict_corners and
// track_smooth_gate_detections -- on a synthetic data set, cameras and markers at the truth.  Prints key = value lines that
// tests/test_gpu_track_smooth_loo.py compares, the pose vector the calls ran at among them (x, 17 digits: exact).
//   usage: smooth_loo_mapper_main <config 1..5> <rw|cv> <sigma_rot> <sigma_trans> <sigma_rot0> <sigma_trans0> <f_max> <cam_id> <marker_id> <time> [...]
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../../automatic-ar_amd/host/multicam_mapper.h"

using namespace aar;

static void line(const char *key, const std::vector<double> &v) {
    printf("%s =", key);
    for (double a : v) printf(" %.17g", a);
    printf("\n");
}

static void line(const char *key, const std::vector<uint8_t> &v) {
    printf("%s =", key);
    for (uint8_t a : v) printf(" %d", (int)a);
    printf("\n");
}

int main(int argc, char **argv) {
    if (argc < 11 || (argc - 8) % 3) return 64;
    aar_synth_desc sd;
    aar_synth_default(&sd, atoi(argv[1]));
    aar_dataset *d = nullptr;
    if (aar_synth_generate(&sd, &d)) { fprintf(stderr, "%s\n", aar_last_error()); return 1; }
    memcpy(d->x_full, d->x_truth, sizeof(double) * 6 * (size_t)(d->num_cams - 1 + d->num_markers - 1));
    const int model = strcmp(argv[2], "cv") ? AAR_SMOOTH_MODEL_RANDOM_WALK : AAR_SMOOTH_MODEL_CONSTANT_VELOCITY;
    const double sr = atof(argv[3]), st = atof(argv[4]), sr0 = atof(argv[5]), st0 = atof(argv[6]), f_max = atof(argv[7]);
    std::vector<int> cams, markers;
    std::vector<double> times;
    for (int i = 8; i + 2 < argc; i += 3) { cams.push_back(atoi(argv[i])); markers.push_back(atoi(argv[i + 1])); times.push_back(atof(argv[i + 2])); }
    try {
        MultiCamMapper a(d);   // takes ownership
        a.solver_params.verbose = false;
        a.set_optmize_flag_cam_intrinsics(false);
        a.track();
        a.track_smooth(sr, st, model, sr0, st0);
        MultiCamMapper::SmoothLeverage lv;
        a.track_smooth_detection_leverage(sr, st, model, sr0, st0, lv);
        MultiCamMapper::SmoothLoo lo;
        a.track_smooth_detection_loo(sr, st, model, sr0, st0, f_max, lo);
        MultiCamMapper::SmoothCorners pc, gt;
        a.track_smooth_predict_corners(sr, st, model, sr0, st0, cams, markers, times, pc);
        std::vector<float> obs(pc.uv.size());
        for (size_t i = 0; i < obs.size(); i++) obs[i] = (float)(pc.uv[i] + ((i % 3) - 1.0) * 0.5);
        a.track_smooth_gate_detections(sr, st, model, sr0, st0, cams, markers, times, obs, gt);
        const aar_dataset *ds = a.dataset();
        printf("x =");
        for (int64_t i = 0; i < aar_dataset_full_len(ds); i++) printf(" %.17g", ds->x_full[i]);
        printf("\n");
        printf("rejected = %lld\nundetermined = %lld\nargmax_f = %lld\nsigma2 = %.17g\nlaunches = %d\n", (long long)lo.report.rejected,
               (long long)lo.report.undetermined, (long long)lo.report.argmax_f, lo.report.sigma2, lo.report.launches);
        line("leverage", lv.leverage);
        line("rows", lv.row_leverage);
        line("F", lo.F);
        line("q", lo.q);
        line("keep", lo.keep);
        line("uv", pc.uv);
        line("cov", pc.cov);
        line("status", pc.status);
        std::vector<double> ob(obs.begin(), obs.end());
        line("obs", ob);
        line("innovation", gt.uv);
        line("m2", gt.m2);
        // an id that does not exist is refused by name
        try {
            a.track_smooth_predict_corners(sr, st, model, sr0, st0, {1 << 20}, {markers[0]}, {times[0]}, pc);
            printf("bad_id = accepted\n");
        } catch (const std::invalid_argument &e) {
            printf("bad_id = %s\n", e.what());
        }
    } catch (const std::exception &e) {
        fprintf(stderr, "exception: %s\n", e.what());
        return 2;
    }
    return 0;
}
