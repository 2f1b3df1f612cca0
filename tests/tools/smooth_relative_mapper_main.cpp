// Test driver (not part of the product): MultiCamMapper::track(), track_smooth() under the given motion model and then
// track_smooth_relative() on a synthetic data set, cameras and markers at the truth, for the given pairs of frame indices.  Prints
// key = value lines that tests/test_gpu_track_smooth_relative.py compares, the pose vector the call ran at among them (x, 17 digits: exact).
//   usage: smooth_relative_mapper_main <config 1..5> <rw|cv> <sigma_rot> <sigma_trans> <sigma_rot0> <sigma_trans0> <a> <b> [<a> <b> ...]
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../../automatic-ar_amd/host/multicam_mapper.h"

using namespace aar;

int main(int argc, char **argv) {
    if (argc < 9 || (argc - 7) % 2) return 64;
    aar_synth_desc sd;
    aar_synth_default(&sd, atoi(argv[1]));
    aar_dataset *d = nullptr;
    if (aar_synth_generate(&sd, &d)) { fprintf(stderr, "%s\n", aar_last_error()); return 1; }
    memcpy(d->x_full, d->x_truth, sizeof(double) * 6 * (size_t)(d->num_cams - 1 + d->num_markers - 1));
    const int model = strcmp(argv[2], "cv") ? AAR_SMOOTH_MODEL_RANDOM_WALK : AAR_SMOOTH_MODEL_CONSTANT_VELOCITY;
    const double sr = atof(argv[3]), st = atof(argv[4]), sr0 = atof(argv[5]), st0 = atof(argv[6]);
    std::vector<std::pair<int32_t, int32_t>> pairs;
    for (int i = 7; i + 1 < argc; i += 2) pairs.push_back({atoi(argv[i]), atoi(argv[i + 1])});
    try {
        MultiCamMapper a(d);   // takes ownership
        a.solver_params.verbose = false;
        a.set_optmize_flag_cam_intrinsics(false);
        a.track();
        a.track_smooth(sr, st, model, sr0, st0);
        MultiCamMapper::SmoothRelative q;
        a.track_smooth_relative(sr, st, model, sr0, st0, pairs, q);
        const aar_smooth_relative_report &r = q.report;
        printf("pairs = %d\ndirect = %d\nchained = %d\nmax_lag = %d\nlaunches = %d\nsigma2 = %.17g\n", r.num_pairs, r.num_direct, r.num_chained, r.max_lag,
               r.launches, r.sigma2);
        const aar_dataset *ds = a.dataset();
        printf("x =");
        for (int64_t i = 0; i < aar_dataset_full_len(ds); i++) printf(" %.17g", ds->x_full[i]);
        printf("\n");
        for (size_t k = 0; k < pairs.size(); k++) {
            printf("cross%zu =", k);
            for (int i = 0; i < 36; i++) printf(" %.17g", q.cross_cov[36 * k + i]);
            printf("\nrel%zu =", k);
            for (int i = 0; i < 6; i++) printf(" %.17g", q.rel[6 * k + i]);
            printf("\nrelcov%zu =", k);
            for (int i = 0; i < 36; i++) printf(" %.17g", q.rel_cov[36 * k + i]);
            printf("\n");
        }
    } catch (const std::exception &e) {
        fprintf(stderr, "exception: %s\n", e.what());
        return 2;
    }
    return 0;
}
