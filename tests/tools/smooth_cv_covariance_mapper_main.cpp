// Test driver (not part of the product): MultiCamMapper::track(), track_smooth() under constant velocity and then the track_smooth_covariance()
// overload that takes the model, on a synthetic data set, cameras and markers at the truth; then the same overload under the random walk.
// Prints key = value lines that tests/test_gpu_track_smooth_cv_covariance.py compares.
//   usage: smooth_cv_covariance_mapper_main <config 1..5> <sigma_rot> <sigma_trans> <sigma_rot0> <sigma_trans0>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../../automatic-ar_amd/host/multicam_mapper.h"

using namespace aar;

static void print_block(const char *name, size_t f, const double *b) {
    printf("%s%zu =", name, f);
    for (int i = 0; i < 36; i++) printf(" %.17g", b[i]);
    printf("\n");
}

int main(int argc, char **argv) {
    if (argc < 6) return 64;
    aar_synth_desc sd;
    aar_synth_default(&sd, atoi(argv[1]));
    aar_dataset *d = nullptr;
    if (aar_synth_generate(&sd, &d)) { fprintf(stderr, "%s\n", aar_last_error()); return 1; }
    memcpy(d->x_full, d->x_truth, sizeof(double) * 6 * (size_t)(d->num_cams - 1 + d->num_markers - 1));
    const double sr = atof(argv[2]), st = atof(argv[3]), sr0 = atof(argv[4]), st0 = atof(argv[5]);
    try {
        MultiCamMapper a(d);   // takes ownership
        a.solver_params.verbose = false;
        a.set_optmize_flag_cam_intrinsics(false);
        a.track();
        a.track_smooth(sr, st, AAR_SMOOTH_MODEL_CONSTANT_VELOCITY, sr0, st0);
        MultiCamMapper::SmoothCovariance c;
        a.track_smooth_covariance(sr, st, AAR_SMOOTH_MODEL_CONSTANT_VELOCITY, sr0, st0, c);
        const size_t F = c.frame_cov.size() / 36, P = c.lag_cov.size() / 36, Q = c.lag2_cov.size() / 36;
        printf("frames = %zu\npairs = %zu\nlag2 = %zu\nnum_residuals = %lld\nnum_vars = %lld\n", F, P, Q, (long long)c.report.num_residuals,
               (long long)c.report.num_vars);
        printf("data_cost = %.17g\nprior_cost = %.17g\nsigma2 = %.17g\nlaunches = %d\n", c.report.data_cost, c.report.prior_cost, c.report.sigma2,
               c.report.launches);
        for (size_t f = 0; f < F; f++) print_block("S", f, &c.frame_cov[36 * f]);
        for (size_t f = 0; f < P; f++) print_block("R", f, &c.lag_cov[36 * f]);
        for (size_t f = 0; f < Q; f++) print_block("Q", f, &c.lag2_cov[36 * f]);
        // the random walk through the same overload is the five-argument call
        MultiCamMapper::SmoothCovariance r0, r1;
        a.track_smooth_covariance(sr, st, r0);
        a.track_smooth_covariance(sr, st, AAR_SMOOTH_MODEL_RANDOM_WALK, 0.0, 0.0, r1);
        printf("rw_same = %d\nrw_lag2 = %zu\n", (int)(r0.frame_cov == r1.frame_cov && r0.lag_cov == r1.lag_cov), r1.lag2_cov.size());
    } catch (const std::exception &e) {
        fprintf(stderr, "exception: %s\n", e.what());
        return 2;
    }
    return 0;
}
