// Test driver (not part of the product): MultiCamMapper::track(), track_smooth() and then track_smooth_query() on a synthetic data set, cameras and
// markers at the truth, at the given times.  Prints key = value lines that tests/test_gpu_track_smooth_query.py compares.
//   usage: smooth_query_mapper_main <config 1..5> <sigma_rot> <sigma_trans> <time> ...
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../../automatic-ar_amd/host/multicam_mapper.h"

using namespace aar;

int main(int argc, char **argv) {
    if (argc < 4) return 64;
    aar_synth_desc sd;
    aar_synth_default(&sd, atoi(argv[1]));
    aar_dataset *d = nullptr;
    if (aar_synth_generate(&sd, &d)) { fprintf(stderr, "%s\n", aar_last_error()); return 1; }
    memcpy(d->x_full, d->x_truth, sizeof(double) * 6 * (size_t)(d->num_cams - 1 + d->num_markers - 1));
    std::vector<double> times;
    for (int i = 4; i < argc; i++) times.push_back(atof(argv[i]));
    try {
        MultiCamMapper a(d);   // takes ownership
        a.solver_params.verbose = false;
        a.set_optmize_flag_cam_intrinsics(false);
        a.track();
        a.track_smooth(atof(argv[2]), atof(argv[3]));
        MultiCamMapper::SmoothQuery q, poses;
        a.track_smooth_query(atof(argv[2]), atof(argv[3]), times, q);
        a.track_smooth_query(atof(argv[2]), atof(argv[3]), times, poses, /*covariance=*/false);
        const aar_smooth_query_report &r = q.report;
        printf("queries = %d\ninside = %d\non_frame = %d\noutside = %d\nlaunches = %d\npose_launches = %d\nsigma2 = %.17g\n", r.num_queries, r.num_inside,
               r.num_on_frame, r.num_outside, r.launches, poses.report.launches, r.sigma2);
        printf("same_poses = %d\ncov_without = %zu\n", (int)(q.pose == poses.pose && q.segment == poses.segment), poses.cov.size());
        for (size_t k = 0; k < times.size(); k++) {
            printf("segment%zu = %d\npose%zu =", k, q.segment[k], k);
            for (int i = 0; i < 6; i++) printf(" %.17g", q.pose[6 * k + i]);
            printf("\ncov%zu =", k);
            for (int i = 0; i < 36; i++) printf(" %.17g", q.cov[36 * k + i]);
            printf("\n");
        }
    } catch (const std::exception &e) {
        fprintf(stderr, "exception: %s\n", e.what());
        return 2;
    }
    return 0;
}
