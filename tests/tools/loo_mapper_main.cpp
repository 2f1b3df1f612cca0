// Test driver (not part of the product): MultiCamMapper::detection_loo / gate_detections / write_loo_file by id, compiled against
// automatic-ar_amd/host/multicam_mapper.h.  Prints key = value lines for tests/test_loo_layers_host.py and tests/test_gpu_detection_loo.py.
// The ids are mapped to indices before any device is looked for, so the unknown-id lines come out on every machine.
#include <cmath>
#include <cstdio>
#include <stdexcept>
#include <vector>

#include "../../automatic-ar_amd/host/multicam_mapper.h"

using namespace aar;

int main(int argc, char **argv) {
    aar_synth_desc sd;
    aar_synth_default(&sd, 2);
    sd.num_frames = 12;
    aar_dataset *d = nullptr;
    if (aar_synth_generate(&sd, &d)) { fprintf(stderr, "%s\n", aar_last_error()); return 1; }
    const int64_t o = d->num_obs / 2;
    const int cid = d->cam_ids[d->obs_cam[o]], mid = d->marker_ids[d->obs_marker[o]], fid = d->frame_ids[d->obs_frame[o]];
    const std::vector<float> uv(d->obs_uv + 8 * o, d->obs_uv + 8 * o + 8);
    MultiCamMapper m(d);
    m.set_optmize_flag_cam_intrinsics(false);
    const int bad[3][3] = {{cid + 1000, mid, fid}, {cid, mid + 1000, fid}, {cid, mid, fid + 1000}};
    const char *what[3] = {"camera", "marker", "frame"};
    for (int k = 0; k < 3; k++) {
        try {
            m.gate_detections({bad[k][0]}, {bad[k][1]}, {bad[k][2]}, uv);
            printf("unknown_%s = accepted\n", what[k]);
        } catch (const std::invalid_argument &e) {
            printf("unknown_%s = %s\n", what[k], e.what());
        } catch (const std::exception &e) {
            printf("unknown_%s = other: %s\n", what[k], e.what());
        }
    }
    try {
        m.gate_detections({cid}, {mid}, {fid}, std::vector<float>(7, 0.f));
        printf("lengths = accepted\n");
    } catch (const std::invalid_argument &e) {
        printf("lengths = %s\n", e.what());
    }
    try {
        const MultiCamMapper::GateResult g = m.gate_detections({cid}, {mid}, {fid}, uv);
        const MultiCamMapper::DetectionLoo lo = m.detection_loo(1.0);
        const MultiCamMapper::DetectionLeverage lv = m.detection_leverage(false);
        int64_t rejected = 0, same = 0;
        for (size_t i = 0; i < lo.keep.size(); i++) { rejected += !lo.keep[i]; same += lo.leverage[i] == lv.leverage[i]; }
        printf("gate_status = %d\ngate_chi2 = %.17g\ngate_innovation0 = %.17g\nsigma2 = %.17g\n", (int)g.status[0], g.chi2[0], g.innovation[0], g.report.sigma2);
        printf("detections = %zu\nresid = %zu\nrejected = %lld\nreport_rejected = %lld\nleverage_same = %lld\nF_o = %.17g\nq_o = %.17g\nresid_o0 = %.17g\nmax_f = %.17g\n",
               lo.F.size(), lo.loo_resid.size(), (long long)rejected, (long long)lo.report.rejected, (long long)same, lo.F[o], lo.q[o], lo.loo_resid[8 * o],
               lo.report.max_f);
        if (argc > 1) printf("written = %d\n", (int)m.write_loo_file(argv[1], lo));
    } catch (const std::exception &e) {
        printf("device = %s\n", e.what());
        return 2;
    }
    return 0;
}
