// Test driver (not part of the product): MultiCamMapper::track() and then fit_smooth_sigmas() under the constant-velocity prior on a synthetic
// data set, cameras and markers at the truth.  Prints key = value lines that tests/test_gpu_smooth_cv_fit.py compares.
//   usage: smooth_cv_fit_mapper_main <config 1..5> <sigma_rot> <sigma_trans> <sigma_rot0> <sigma_trans0>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../../automatic-ar_amd/host/multicam_mapper.h"

using namespace aar;

int main(int argc, char **argv) {
    if (argc < 6) return 64;
    aar_synth_desc sd;
    aar_synth_default(&sd, atoi(argv[1]));
    aar_dataset *d = nullptr;
    if (aar_synth_generate(&sd, &d)) { fprintf(stderr, "%s\n", aar_last_error()); return 1; }
    memcpy(d->x_full, d->x_truth, sizeof(double) * 6 * (size_t)(d->num_cams - 1 + d->num_markers - 1));
    const size_t n0 = 6 * (size_t)(d->num_cams - 1 + d->num_markers - 1), F = (size_t)d->num_frames;
    try {
        MultiCamMapper a(d);   // takes ownership
        a.solver_params.verbose = false;
        a.set_optmize_flag_cam_intrinsics(false);
        a.track();
        MultiCamMapper::SmoothFit fit;
        a.fit_smooth_sigmas(atof(argv[2]), atof(argv[3]), AAR_SMOOTH_MODEL_CONSTANT_VELOCITY, atof(argv[4]), atof(argv[5]), fit);
        const aar_smooth_fit_report &r = fit.report;
        printf("iterations = %d\nstop_code = %d\nlm_steps = %d\nrows = %zu\n", r.iterations, r.stop_code, r.lm_steps, fit.path.size() / 3);
        printf("sigma_px = %.17g\nsigma_rot = %.17g\nsigma_trans = %.17g\nsigma_rot_eff = %.17g\nsigma_trans_eff = %.17g\n", r.sigma_px, r.sigma_rot,
               r.sigma_trans, r.sigma_rot_eff, r.sigma_trans_eff);
        printf("path =");
        for (double v : fit.path) printf(" %.17g", v);
        printf("\nz =");
        for (size_t i = 0; i < 6 * F; i++) printf(" %.17g", d->x_full[n0 + i]);
        printf("\n");
    } catch (const std::exception &e) {
        fprintf(stderr, "exception: %s\n", e.what());
        return 2;
    }
    return 0;
}
