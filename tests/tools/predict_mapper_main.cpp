// Test driver (not part of the product): MultiCamMapper::predict_corners / detection_leverage by id, compiled against the mirror of
// automatic-ar_amd/host/multicam_mapper.h.  Prints key = value lines for tests/test_predict_host.py and tests/test_gpu_predict_corners.py.
// The ids are mapped to indices before any device is looked for, so the unknown-id lines come out on every machine.
#include <cmath>
#include <cstdio>
#include <stdexcept>
#include <vector>

#include "../../automatic-ar_amd/host/multicam_mapper.h"

using namespace aar;

int main() {
    aar_synth_desc sd;
    aar_synth_default(&sd, 2);
    sd.num_frames = 12;
    aar_dataset *d = nullptr;
    if (aar_synth_generate(&sd, &d)) { fprintf(stderr, "%s\n", aar_last_error()); return 1; }
    const int64_t o = d->num_obs / 2;   // (a detection's own triple: seen, so its covariance is defined)
    const int cid = d->cam_ids[d->obs_cam[o]], mid = d->marker_ids[d->obs_marker[o]], fid = d->frame_ids[d->obs_frame[o]];
    MultiCamMapper m(d);
    m.set_optmize_flag_cam_intrinsics(false);
    const int bad[3][3] = {{cid + 1000, mid, fid}, {cid, mid + 1000, fid}, {cid, mid, fid + 1000}};
    const char *what[3] = {"camera", "marker", "frame"};
    for (int k = 0; k < 3; k++) {
        try {
            m.predict_corners({cid, bad[k][0]}, {mid, bad[k][1]}, {fid, bad[k][2]});
            printf("unknown_%s = accepted\n", what[k]);
        } catch (const std::invalid_argument &e) {
            printf("unknown_%s = %s\n", what[k], e.what());
        } catch (const std::exception &e) {
            printf("unknown_%s = other: %s\n", what[k], e.what());
        }
    }
    try {
        m.predict_corners({cid}, {mid, mid}, {fid});
        printf("lengths = accepted\n");
    } catch (const std::invalid_argument &e) {
        printf("lengths = %s\n", e.what());
    }
    try {
        const MultiCamMapper::CornerPrediction p = m.predict_corners({cid, d->cam_ids[d->obs_cam[0]]}, {mid, d->marker_ids[d->obs_marker[0]]}, {fid, d->frame_ids[d->obs_frame[0]]});
        const MultiCamMapper::CornerPrediction q = m.predict_corners({cid}, {mid}, {fid}, false);
        const MultiCamMapper::DetectionLeverage lv = m.detection_leverage(true);
        double sum = 0;
        for (double h : lv.leverage) sum += h;
        printf("queries = %zu\nstatus0 = %d\nuv0 = %.17g\nuv0_nocov = %.17g\ncov00 = %.17g\nsigma2 = %.17g\n", p.status.size(), (int)p.status[0], p.uv[0], q.uv[0],
               p.cov[0], p.report.sigma2);
        printf("leverages = %zu\nrows = %zu\nleverage_sum = %.17g\nreport_sum = %.17g\nnum_live_vars = %lld\n", lv.leverage.size(), lv.row_leverage.size(), sum,
               lv.report.leverage_sum, (long long)lv.report.num_live_vars);
    } catch (const std::exception &e) {
        printf("device = %s\n", e.what());
        return 2;
    }
    return 0;
}
