// aar_find_solution: the find_solution driver for the accelerated path (apps/find_solution.cpp:28-181).
//
//   aar_find_solution <data_folder> <marker_size> [ignored] [-subseqs] [-exclude-cams ...] [-with-huber] [-thresh t] [-solver direct|spcg|pcg|auto]
//
// File contract kept from the reference (:45,99-100,146-147,162-163,175-177): reads <folder>/aruco.detections and
// <folder>/<cam>/calib.{xml,yml,yaml}, runs the Initializer (IPPE poses, votes, spanning trees -- on the GPU, aar_initializer_run),
// writes <folder>/initial<suffix>.solution(.yaml), solves, writes <folder>/final<suffix>.solution(.yaml) and prints
// "The algorithm took: ...".  With -from-initial, or when the folder holds no calibration, it starts from an existing
// initial<suffix>.solution instead (e.g. one the reference wrote).  A synthetic folder in the reference's formats:
//   aar_find_solution --synth <config 1..5> <out_folder>
#include <sys/stat.h>

#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <memory>
#include <set>
#include <stdexcept>
#include <string>
#include <vector>

#include "multicam_mapper.h"
#include "se3.h"

using namespace std;

static int print_usage(const char *a0) {
    cout << "Usage: " << a0 << " <data_folder_path> <marker_size> [ignored] [-subseqs] [-exclude-cams <cam_id> ...] [-with-huber] [-thresh <t>] [-from-initial] [-solver direct|spcg|pcg|auto] [-covariance] [-leverage <h_min>] [-residuals] [-reject-outliers <k> [-reject-min-px <px>]] [-fix-cams <id>[,<id>...]] [-fix-markers <id>[,<id>...]] [-prior-solution <file> [-prior-sigma-deg <d>] [-prior-sigma-m <m>]] [-relative-prior-solution <file> [-relative-kinds cams|markers|both] [-relative-sigma-deg <d>] [-relative-sigma-m <m>]] [-tracking-only -smooth <sigma_rot> <sigma_trans> [-cv <sigma_rot0> <sigma_trans0> [-cv-covariance] [-cv-fit-sigmas] [-cv-resample <n>]] [-smooth-covariance] [-fit-sigmas] [-resample <n>] [-relative-to <frame_id>] [-smooth-loo <f_max>] [-smooth-reject-loo <f_max>]] [-tracking-only -live <lag> [<sigma_rot> <sigma_trans>] [-from-detections [vote|best]] [-anchor fixed|marginal] [-live-covariance] [-gate <k_median> <min_px>] [-motion cv|rw [<max_dt>]]]" << endl;
    cout << "       -covariance          also write final.covariance.yaml (pose covariance of the final solution)" << endl;
    cout << "       -leverage <h_min>    also write final.leverage.yaml (leverage of every detection, 0 .. 8; those from h_min up are listed)" << endl;
    cout << "       -residuals           also write final.residuals.yaml (reprojection errors per camera and marker)" << endl;
    cout << "       -loo <f_max>         also write final.loo.yaml (leave-one-out F of every detection; those above f_max or undetermined are listed)" << endl;
    cout << "       -reject-loo <f_max>  after the solve, drop of every frame the detection with the largest F above f_max and solve again (not with -with-huber)" << endl;
    cout << "       -smooth-loo <f_max>  (needs -smooth) also write final.smooth_loo.yaml (leave-one-out F of every detection against the smoothed track)" << endl;
    cout << "       -smooth-reject-loo <f_max>   (needs -smooth) drop of every frame the detection with the largest F above f_max and smooth again (up to 3 rounds)" << endl;
    cout << "       -reject-outliers k   after the solve, drop the detections whose error exceeds max(px, k * median) and solve again" << endl;
    cout << "                            (up to 3 rounds, until a round drops nothing); final.solution keeps the remaining detections" << endl;
    cout << "       -reject-min-px px    the floor of that threshold in pixels (default 0)" << endl;
    cout << "       -fix-cams ids        hold these cameras exactly where the initial solution has them (comma-separated ids)" << endl;
    cout << "       -fix-markers ids     the same for markers" << endl;
    cout << "       -prior-solution f    pull every non-root camera and marker of the .solution file f toward its pose there (isotropic" << endl;
    cout << "                            prior, information diag(1/sigma_rot^2 x3, 1/sigma_t^2 x3)); f must have the same root camera and marker ids" << endl;
    cout << "       -prior-sigma-deg d   rotation sigma of those priors in degrees (default 1)" << endl;
    cout << "       -prior-sigma-m m     translation sigma of those priors in metres (default 0.01)" << endl;
    cout << "       -relative-prior-solution f   hold the RELATIVE poses of the .solution file f: a chain of pair priors between consecutive cameras /" << endl;
    cout << "                            markers (ascending problem index) that f has, each an isotropic prior on T_a^-1 T_b; f may have other roots" << endl;
    cout << "       -relative-kinds k    cams | markers | both (default both)" << endl;
    cout << "       -relative-sigma-deg d, -relative-sigma-m m   sigmas of those priors (defaults 1 degree, 0.01 m)" << endl;
    cout << "       " << a0 << " --synth <config 1..5> <out_folder>   (write a synthetic data set in the reference's file formats)" << endl;
    return -1;
}

static int synth(int cfg, const string &folder) {
    aar_synth_desc sd;
    aar_synth_default(&sd, cfg);
    aar_dataset *d = nullptr;
    if (aar_synth_generate(&sd, &d)) { cerr << aar_last_error() << endl; return 1; }
    mkdir(folder.c_str(), 0755);
    int rc = aar_detections_write((folder + "/aruco.detections").c_str(), d);
    for (int c = 0; c < d->num_cams && !rc; c++) {  // one calib.yml per camera slot, cv::FileStorage YAML dialect
        char dir[64];
        snprintf(dir, sizeof dir, "/cam_%03d", d->cam_ids[c]);
        mkdir((folder + dir).c_str(), 0755);
        FILE *f = fopen((folder + dir + "/calib.yml").c_str(), "w");
        if (!f) { rc = 1; break; }
        const double *K = d->cam_mats + 9 * c;
        fprintf(f, "%%YAML:1.0\n---\nimage_width: %d\nimage_height: %d\ncamera_matrix: !!opencv-matrix\n   rows: 3\n   cols: 3\n   dt: d\n   data: [ ",
                d->image_sizes[2 * c], d->image_sizes[2 * c + 1]);
        for (int i = 0; i < 9; i++) fprintf(f, "%.17g%s", K[i], i < 8 ? ", " : " ]\n");
        fprintf(f, "distortion_coefficients: !!opencv-matrix\n   rows: 1\n   cols: 5\n   dt: d\n   data: [ 0., 0., 0., 0., 0. ]\n");
        fclose(f);
    }
    rc |= aar_solution_write((folder + "/initial.solution").c_str(), d);
    rc |= aar_solution_write_yaml((folder + "/initial.solution.yaml").c_str(), d);
    if (rc) cerr << aar_last_error() << endl;
    cout << "wrote " << folder << ": cams=" << d->num_cams << " markers=" << d->num_markers << " frames=" << d->num_frames
         << " marker-observations=" << d->num_obs << endl;
    aar_dataset_free(d);
    return rc ? 1 : 0;
}

// comma-separated ids of -fix-cams / -fix-markers; false on anything that is not an integer list
static bool parse_ids(const string &a, set<int> &out) {
    size_t p = 0;
    while (p <= a.size()) {
        const size_t q = a.find(',', p);
        const string tok = a.substr(p, q == string::npos ? string::npos : q - p);
        char *end = nullptr;
        const long v = strtol(tok.c_str(), &end, 10);
        if (tok.empty() || *end != '\0') return false;
        out.insert((int)v);
        if (q == string::npos) break;
        p = q + 1;
    }
    return true;
}

// -prior-solution: an isotropic prior on every non-root camera and marker of the file; its roots must be the problem's (the poses are relative to them)
static int read_pose_priors(const string &path, const aar_dataset *d, double sigma_deg, double sigma_m, vector<aar::MultiCamMapper::PosePrior> &out) {
    aar_dataset *p = nullptr;
    if (aar_solution_read(path.c_str(), &p)) {
        cerr << "cannot read the prior solution " << path << ": " << aar_last_error() << endl;
        return 1;
    }
    std::unique_ptr<aar_dataset, void (*)(aar_dataset *)> hold(p, aar_dataset_free);
    if (p->cam_ids[p->root_cam] != d->cam_ids[d->root_cam] || p->marker_ids[p->root_marker] != d->marker_ids[d->root_marker]) {
        cerr << "the prior solution " << path << " has root camera " << p->cam_ids[p->root_cam] << " / marker " << p->marker_ids[p->root_marker]
             << ", the problem " << d->cam_ids[d->root_cam] << " / " << d->marker_ids[d->root_marker] << endl;
        return 1;
    }
    const double sr = sigma_deg * M_PI / 180.0;
    aar::MultiCamMapper::Mat66 info{};
    for (int i = 0; i < 6; i++) info[7 * i] = i < 3 ? 1.0 / (sr * sr) : 1.0 / (sigma_m * sigma_m);
    auto add = [&](int kind, int id, const double *x6) {
        const aar::Rigid r = aar::pose_to_rigid(x6);
        aar::MultiCamMapper::PosePrior q;
        q.kind = kind;
        q.id = id;
        for (int i = 0; i < 3; i++) {
            for (int j = 0; j < 3; j++) q.T[4 * i + j] = r.R[3 * i + j];
            q.T[4 * i + 3] = r.t[i];
        }
        q.T[15] = 1.0;
        q.info = info;
        out.push_back(q);
    };
    // x_full: (C-1) cameras | (M-1) markers, ascending index, roots skipped
    for (int c = 0, k = 0; c < p->num_cams; c++)
        if (c != p->root_cam) add(AAR_PRIOR_CAMERA, p->cam_ids[c], p->x_full + 6 * (k++));
    for (int m = 0, k = 0; m < p->num_markers; m++)
        if (m != p->root_marker) add(AAR_PRIOR_MARKER, p->marker_ids[m], p->x_full + 6 * (size_t)(p->num_cams - 1) + 6 * (k++));
    return 0;
}

// -relative-prior-solution: a chain of pair priors between consecutive cameras / markers of the problem (ascending index) that the file has, each
// T_a^-1 T_b of the file's poses with an isotropic information matrix.  Relative poses do not depend on the roots, so the file may have its own.
static int read_relative_priors(const string &path, const aar_dataset *d, int kinds, double sigma_deg, double sigma_m, vector<aar::MultiCamMapper::RelativePrior> &out) {
    aar_dataset *p = nullptr;
    if (aar_solution_read(path.c_str(), &p)) {
        cerr << "cannot read the relative prior solution " << path << ": " << aar_last_error() << endl;
        return 1;
    }
    std::unique_ptr<aar_dataset, void (*)(aar_dataset *)> hold(p, aar_dataset_free);
    const double sr = sigma_deg * M_PI / 180.0;
    aar::MultiCamMapper::Mat66 info{};
    for (int i = 0; i < 6; i++) info[7 * i] = i < 3 ? 1.0 / (sr * sr) : 1.0 / (sigma_m * sigma_m);
    // the file's pose of entity `idx` of a group of n with root `root` whose x_full block starts at `base`
    auto pose_of = [&](int idx, int root, size_t base) {
        if (idx == root) return aar::Rigid::identity();
        return aar::pose_to_rigid(p->x_full + base + 6 * (size_t)(idx - (idx > root ? 1 : 0)));
    };
    auto chain = [&](int kind, const int32_t *ids, int n, const int32_t *fids, int fn, int froot, size_t base) {
        int prev_id = 0;
        aar::Rigid prev{};
        bool have = false;
        for (int i = 0; i < n; i++) {
            const int32_t *e = fids + fn, *q = std::lower_bound(fids, e, ids[i]);
            if (q == e || *q != ids[i]) continue;
            const aar::Rigid cur = pose_of((int)(q - fids), froot, base);
            if (have) {
                const aar::Rigid rel = aar::compose(aar::inverse(prev), cur);
                aar::MultiCamMapper::RelativePrior r;
                r.kind = kind; r.id_a = prev_id; r.id_b = ids[i];
                for (int a = 0; a < 3; a++) {
                    for (int b = 0; b < 3; b++) r.T[4 * a + b] = rel.R[3 * a + b];
                    r.T[4 * a + 3] = rel.t[a];
                }
                r.T[15] = 1.0;
                r.info = info;
                out.push_back(r);
            }
            prev = cur; prev_id = ids[i]; have = true;
        }
    };
    if (kinds & 1) chain(AAR_PRIOR_CAMERA, d->cam_ids, d->num_cams, p->cam_ids, p->num_cams, p->root_cam, 0);
    if (kinds & 2) chain(AAR_PRIOR_MARKER, d->marker_ids, d->num_markers, p->marker_ids, p->num_markers, p->root_marker, 6 * (size_t)(p->num_cams - 1));
    return 0;
}

// -reject-outliers: report, drop, solve again from that solution -- until a round drops nothing, at most 3 rounds.  final.residuals.yaml
// then holds the final solution's statistics over the detections it kept; its rejected counts and list cover every detection dropped in
// any round (with its error in the round that dropped it), against the detections the first solve had.
static int reject_outliers(aar::MultiCamMapper &mcm, const string &res_path, double k, double min_px) {
    try {
        aar_dataset *d0 = nullptr;   // a copy of the detections before any round
        {
            const aar_dataset *cur = mcm.dataset();
            vector<uint8_t> all(std::max<int64_t>(cur->num_obs, 1), 1);
            if (aar_dataset_select_observations(cur, all.data(), &d0)) throw runtime_error(aar_last_error());
        }
        unique_ptr<aar_dataset, void (*)(aar_dataset *)> hold(d0, aar_dataset_free);
        vector<int64_t> alive(d0->num_obs);   // original index of every detection the mapper still has
        for (int64_t o = 0; o < d0->num_obs; o++) alive[o] = o;
        vector<uint8_t> keep0(std::max<int64_t>(d0->num_obs, 1), 1);
        vector<double> err0(std::max<int64_t>(d0->num_obs, 1), 0.0);
        for (int round = 1; round <= 3; round++) {
            aar::MultiCamMapper::ResidualReport rr;
            const int64_t dropped = mcm.reject_outliers(k, min_px, &rr);
            const aar_residual_report &r = rr.report;
            cout << "outlier round " << round << ": median " << r.median << " px, threshold " << r.threshold << " px, " << dropped << " of " << r.num_detections
                 << " detections rejected" << endl;
            if (r.cams_emptied || r.markers_emptied || r.frames_emptied)
                cerr << "warning: the rejected detections were all of " << r.cams_emptied << " camera(s), " << r.markers_emptied << " marker(s) and "
                     << r.frames_emptied << " frame(s)" << endl;
            vector<int64_t> next;
            for (size_t i = 0; i < rr.keep.size(); i++) {
                if (rr.keep[i]) { next.push_back(alive[i]); continue; }
                keep0[alive[i]] = 0;
                err0[alive[i]] = rr.det_err[i];
            }
            alive.swap(next);
            if (dropped == 0) break;
            mcm.solve();
        }
        aar::MultiCamMapper::ResidualReport fin = mcm.residual_report(nullptr);
        // the rejected counts of the file: every detection dropped in any round, per camera / marker index of the (unchanged) entity lists
        fin.report.num_rejected = 0;
        for (int c = 0; c < d0->num_cams; c++) fin.cam_stats[4 * c + 3] = 0;
        for (int m = 0; m < d0->num_markers; m++) fin.marker_stats[4 * m + 3] = 0;
        for (int64_t o = 0; o < d0->num_obs; o++)
            if (!keep0[o]) { fin.report.num_rejected++; fin.cam_stats[4 * d0->obs_cam[o] + 3]++; fin.marker_stats[4 * d0->obs_marker[o] + 3]++; }
        if (aar_residual_report_write_yaml(res_path.c_str(), d0, fin.cam_stats.data(), fin.marker_stats.data(), err0.data(), keep0.data(), &fin.report))
            throw runtime_error(aar_last_error());
        cout << "residuals: " << fin.report.num_detections << " detections kept, " << fin.report.num_rejected << " rejected, RMSE " << fin.report.rmse
             << " px, written to " << res_path << endl;
    } catch (const exception &e) {
        cerr << "outlier rejection failed: " << e.what() << endl;
        return 1;
    }
    return 0;
}

// -reject-loo: report, drop, solve again from that solution -- until a round drops nothing, at most 3 rounds; a round drops of every frame
// only the detection with the largest F above f_max
static int reject_loo(aar::MultiCamMapper &mcm, double f_max) {
    try {
        for (int round = 1; round <= 3; round++) {
            aar::MultiCamMapper::DetectionLoo loo;
            const aar_dataset *d = mcm.dataset();
            vector<int> fid, cid, mid;   // (ids of the detections before the drop: the data set is rebuilt by it)
            for (int64_t o = 0; o < d->num_obs; o++) {
                fid.push_back(d->frame_ids[d->obs_frame[o]]); cid.push_back(d->cam_ids[d->obs_cam[o]]); mid.push_back(d->marker_ids[d->obs_marker[o]]);
            }
            const int64_t dropped = mcm.reject_loo(f_max, &loo);
            cout << "loo round " << round << ": largest F " << loo.report.max_f << " (f_max " << f_max << "), " << loo.report.undetermined << " undetermined, "
                 << dropped << " of " << loo.F.size() << " detections rejected" << endl;
            for (size_t o = 0; o < loo.keep.size(); o++)
                if (!loo.keep[o])
                    cout << "loo rejected: round " << round << " frame_id " << fid[o] << " cam_id " << cid[o] << " marker_id " << mid[o] << " F " << loo.F[o] << endl;
            if (dropped == 0) break;
            mcm.solve();
        }
    } catch (const exception &e) {
        cerr << "leave-one-out rejection failed: " << e.what() << endl;
        return 1;
    }
    return 0;
}

int main(int argc, char *argv[]) {
    if (argc >= 4 && string(argv[1]) == "--synth") return synth(atoi(argv[2]), argv[3]);
    if (argc < 3) return print_usage(argv[0]);
    const string folder_path = argv[1];
    const double marker_size = stod(argv[2]);
    bool use_subseqs = false, with_huber = false, set_threshold = false, from_initial = false, tracking_only = false;
    bool covariance = false;   // not an option of the reference: -covariance also writes final.covariance.yaml (aar_problem_covariance)
    // nor this: -leverage h_min also writes final.leverage.yaml (aar_problem_detection_leverage): the detections whose
    // leverage is at least h_min are listed with their reprojection error
    bool leverage = false, leverage_set = false;
    double leverage_min = 0.0;
    // nor these: -loo f_max writes final.loo.yaml (aar_problem_detection_loo); -reject-loo f_max mirrors -reject-outliers with
    // the leave-one-out F, one detection per frame and round
    double loo_f_max = 0.0, reject_loo_f = 0.0;
    bool loo = false, reject_loo_on = false;
    bool residuals = false;    // nor these: -residuals writes final.residuals.yaml; -reject-outliers k drops detections above max(min_px, k median) and solves again
    double reject_k = 0.0, reject_min_px = 0.0;
    double threshold = 2.0;
    set<int> excluded_cams;
    // nor these: -fix-cams / -fix-markers hold entities by id, -prior-solution pulls the cameras and markers toward a solution file's poses
    set<int> fixed_cams, fixed_markers;
    bool fix_cams = false, fix_markers = false;
    string prior_path;
    double prior_sigma_deg = 1.0, prior_sigma_m = 0.01;
    // nor these: -relative-prior-solution holds the relative poses of consecutive cameras / markers of a solution file (pair priors)
    string rel_path;
    int rel_kinds = 3;   // bit 0: cameras, bit 1: markers
    double rel_sigma_deg = 1.0, rel_sigma_m = 0.01;
    // nor this: -smooth <sigma_rot> <sigma_trans> (only with -tracking-only) refines every frame with track() after the solve and then smooths the
    // trajectory with a motion prior between consecutive frames (MultiCamMapper::track_smooth)
    bool smooth = false;
    double smooth_sigma[2] = {0.0, 0.0};
    int smooth_args = 0;
    // ... -smooth-covariance (only with -smooth) also writes every frame's 6x6 pose covariance at the smoothed poses to
    // final.smooth_covariance.yaml (MultiCamMapper::track_smooth_covariance)
    bool smooth_covariance = false;
    // ... -cv <sigma_rot0> <sigma_trans0> (only with -smooth) smooths under the constant-velocity prior: the -smooth sigmas
    // bound the deviation from constant velocity, these two the first pair's motion.  Not with -smooth-covariance, -fit-sigmas or -resample
    // (the fit under this prior is -cv-fit-sigmas)
    bool smooth_cv = false;
    // ... -cv-covariance (only with -smooth and -cv) writes final.smooth_covariance.yaml under the constant-velocity prior, in -smooth-covariance's
    // format (MultiCamMapper::track_smooth_covariance with the model)
    bool cv_covariance = false;
    // ... -cv-fit-sigmas (only with -smooth and -cv) first fits the corner noise and the two -smooth sigmas under the constant-velocity prior, the
    // -cv sigmas held as physical values (MultiCamMapper::fit_smooth_sigmas with the model), and smooths with the fitted
    // effective values and the -cv sigmas over the fitted corner noise
    bool cv_fit_sigmas = false;
    double smooth_sigma0[2] = {0.0, 0.0};
    int smooth_cv_args = 0;
    // ... -fit-sigmas (only with -smooth) first fits the corner noise and the two sigmas to the sequence, from the given values as the start
    // (MultiCamMapper::fit_smooth_sigmas), and smooths with the fitted effective values
    bool fit_sigmas = false;
    // ... -resample <n> (only with -smooth, n >= 2) also writes the smoothed track at n points per gap of frame ids, the frames included, with
    // pose and 6x6 covariance to final.resampled.yaml (MultiCamMapper::track_smooth_query)
    bool resample = false;
    int resample_n = 0;
    // ... -cv-resample <n> (only with -smooth and -cv, n >= 2) writes final.resampled.yaml under the constant-velocity prior, in -resample's format
    // (MultiCamMapper::track_smooth_query with the model)
    bool cv_resample = false;
    // ... -relative-to <frame_id> (only with -smooth; with -cv under the constant-velocity prior) also writes every frame's motion relative to
    // that frame -- rel = [log(R_a^T R_b); t_b - t_a], its 6x6 covariance sigma2 * rel_cov and the baseline time -- to
    // final.smooth_relative.yaml (MultiCamMapper::track_smooth_relative), at the poses of the solution file written beside it
    bool relative_to = false, relative_set = false;
    long relative_id = 0;
    // ... -smooth-loo <f_max> (only with -smooth; with -cv under the constant-velocity prior) writes the smoothed track's leave-one-out report to
    // final.smooth_loo.yaml (MultiCamMapper::track_smooth_detection_loo); -smooth-reject-loo <f_max> drops of every frame the
    // detection with the largest F above f_max and smooths again, at most 3 rounds: -reject-loo on the smoothed track
    double smooth_loo_f = 0.0, smooth_reject_loo_f = 0.0;
    bool smooth_loo = false, smooth_reject_loo = false;
    // nor this: -live <lag> [sigma_rot sigma_trans] (only with -tracking-only) takes the cameras and markers as they are and feeds the frames one at a
    // time through the live tracker (MultiCamMapper::track_live) instead of solving; without sigmas there is no prior and the lag must be 0
    // ... with -from-detections [vote|best] the frames are fed the RAW detections of aruco.detections (calib.* for the lenses) and start from their
    // own vote, as apps/track.cpp does; the solution file's object poses are not read and the Initializer does not run
    bool live = false, from_detections = false;
    int start_policy = AAR_TRACKER_START_VOTE;
    int live_lag = -1, live_args = 0;
    // ... -anchor marginal marginalises the frame that leaves the window instead of freezing it (needs the sigmas and a lag >= 1); -live-covariance
    // also writes every frame's lagged 6x6 covariance block and sigma2 to final<name>.covariance.yaml beside the poses
    int live_anchor = AAR_TRACKER_ANCHOR_FIXED;
    bool live_anchor_set = false, live_covariance = false;
    double live_sigma[2] = {0.0, 0.0};
    // ... -gate <k_median> <min_px> gates every pushed frame on the device with the batch path's outlier rule (-reject-outliers / -reject-min-px)
    // at the pose the push starts from; one of the two may be 0
    bool live_gate = false;
    int gate_args = 0;
    double gate_v[2] = {0.0, 0.0};
    // ... -motion cv [<max_dt>] gives every pair the motion expected from the two newest estimates, constant velocity (needs
    // the sigmas); no prediction across a gap of frame ids above max_dt (0 or absent: no limit); -motion rw is the default, the random walk
    bool live_motion = false;
    int motion_args = 0, motion_model = AAR_TRACKER_MOTION_RANDOM_WALK;
    double motion_max_dt = 0.0;
    int solver = AAR_SOLVER_AUTO;   // not an option of the reference: how the damped systems are solved (aar_solver_options); `-solver direct` = the reference's every step
    enum ArgFlag { NONE, ExcludeCams, Threshold, Solver, RejectK, RejectPx, FixCams, FixMarkers, PriorPath, PriorDeg, PriorM, RelPath, RelKinds, RelDeg, RelM, Smooth, SmoothCv, Resample, RelativeTo, Live, Anchor, Gate, Motion, Leverage, Loo, RejectLoo, SmoothLoo, SmoothRejectLoo } arg_flag = NONE;
    for (int i = 4; i < argc; i++) {  // sic: the reference starts at argv[4] (apps/find_solution.cpp:47)
        const string a = argv[i];
        if (a == "-subseqs") use_subseqs = true;
        else if (a == "-exclude-cams") arg_flag = ExcludeCams;
        else if (a == "-with-huber") { with_huber = true; arg_flag = NONE; }
        else if (a == "-from-initial") { from_initial = true; arg_flag = NONE; }
        else if (a == "-tracking-only") { tracking_only = true; arg_flag = NONE; }   // names the files only, as in the reference (:54-57,76-77)
        else if (a == "-thresh") { set_threshold = true; arg_flag = Threshold; }
        else if (a == "-solver") arg_flag = Solver;
        else if (a == "-covariance") { covariance = true; arg_flag = NONE; }
        else if (a == "-leverage") { leverage = true; arg_flag = Leverage; }
        else if (a == "-loo") { loo = true; arg_flag = Loo; }
        else if (a == "-reject-loo") { reject_loo_on = true; arg_flag = RejectLoo; }
        else if (a == "-smooth-loo") { smooth_loo = true; arg_flag = SmoothLoo; }
        else if (a == "-smooth-reject-loo") { smooth_reject_loo = true; arg_flag = SmoothRejectLoo; }
        else if (a == "-residuals") { residuals = true; arg_flag = NONE; }
        else if (a == "-reject-outliers") arg_flag = RejectK;
        else if (a == "-reject-min-px") arg_flag = RejectPx;
        else if (a == "-fix-cams") arg_flag = FixCams;
        else if (a == "-fix-markers") arg_flag = FixMarkers;
        else if (a == "-prior-solution") arg_flag = PriorPath;
        else if (a == "-prior-sigma-deg") arg_flag = PriorDeg;
        else if (a == "-prior-sigma-m") arg_flag = PriorM;
        else if (a == "-relative-prior-solution") arg_flag = RelPath;
        else if (a == "-relative-kinds") arg_flag = RelKinds;
        else if (a == "-relative-sigma-deg") arg_flag = RelDeg;
        else if (a == "-relative-sigma-m") arg_flag = RelM;
        else if (a == "-smooth") { smooth = true; smooth_args = 0; arg_flag = Smooth; }
        else if (a == "-smooth-covariance") { smooth_covariance = true; arg_flag = NONE; }
        else if (a == "-cv") { smooth_cv = true; smooth_cv_args = 0; arg_flag = SmoothCv; }
        else if (a == "-cv-covariance") { cv_covariance = true; arg_flag = NONE; }
        else if (a == "-cv-fit-sigmas") { cv_fit_sigmas = true; arg_flag = NONE; }
        else if (a == "-fit-sigmas") { fit_sigmas = true; arg_flag = NONE; }
        else if (a == "-resample") { resample = true; resample_n = 0; arg_flag = Resample; }
        else if (a == "-cv-resample") { cv_resample = true; resample_n = 0; arg_flag = Resample; }
        else if (a == "-relative-to") { relative_to = true; relative_set = false; arg_flag = RelativeTo; }
        else if (a == "-live") { live = true; live_args = 0; arg_flag = Live; }
        else if (a == "-anchor") { live_anchor_set = true; arg_flag = Anchor; }
        else if (a == "-live-covariance") { live_covariance = true; arg_flag = NONE; }
        else if (a == "-gate") { live_gate = true; gate_args = 0; arg_flag = Gate; }
        else if (a == "-motion") { live_motion = true; motion_args = 0; arg_flag = Motion; }
        else if (arg_flag == Motion && motion_args == 0) {
            if (a != "cv" && a != "rw") return print_usage(argv[0]);
            motion_model = a == "cv" ? AAR_TRACKER_MOTION_CONSTANT_VELOCITY : AAR_TRACKER_MOTION_RANDOM_WALK;
            motion_args = 1;
        }
        else if (arg_flag == Motion && !a.empty() && a[0] != '-') {   // the optional max_dt
            char *end = nullptr;
            const double v = strtod(a.c_str(), &end);
            if (*end != '\0' || !(v >= 0.0) || !std::isfinite(v)) return print_usage(argv[0]);
            motion_max_dt = v;
            motion_args = 2;
            arg_flag = NONE;
        }
        else if (arg_flag == Gate) {
            char *end = nullptr;
            const double v = strtod(a.c_str(), &end);
            if (*end != '\0' || a.empty() || !(v >= 0.0) || !std::isfinite(v)) return print_usage(argv[0]);
            gate_v[gate_args++] = v;
            if (gate_args == 2) arg_flag = NONE;
        }
        else if (arg_flag == Anchor) {
            if (a != "fixed" && a != "marginal") return print_usage(argv[0]);
            live_anchor = a == "marginal" ? AAR_TRACKER_ANCHOR_MARGINAL : AAR_TRACKER_ANCHOR_FIXED;
            arg_flag = NONE;
        }
        else if (a == "-from-detections") {
            from_detections = true; arg_flag = NONE;
            if (i + 1 < argc && (string(argv[i + 1]) == "vote" || string(argv[i + 1]) == "best"))
                start_policy = string(argv[++i]) == "best" ? AAR_TRACKER_START_BEST : AAR_TRACKER_START_VOTE;
        }
        else if (arg_flag == Live) {
            char *end = nullptr;
            if (live_args == 0) {
                const long v = strtol(a.c_str(), &end, 10);
                if (*end != '\0' || a.empty() || v < 0 || v > AAR_TRACKER_MAX_LAG) return print_usage(argv[0]);
                live_lag = (int)v;
                live_args = 1;
            } else {
                const double v = strtod(a.c_str(), &end);
                if (*end != '\0' || !(v > 0.0) || !std::isfinite(v)) return print_usage(argv[0]);
                live_sigma[live_args++ - 1] = v;
                if (live_args == 3) arg_flag = NONE;
            }
        }
        else if (arg_flag == Resample) {
            char *end = nullptr;
            const long v = strtol(a.c_str(), &end, 10);
            if (*end != '\0' || a.empty() || v < 2 || v > 1000000) return print_usage(argv[0]);
            resample_n = (int)v;
            arg_flag = NONE;
        }
        else if (arg_flag == RelativeTo) {
            char *end = nullptr;
            relative_id = strtol(a.c_str(), &end, 10);
            if (*end != '\0' || a.empty()) return print_usage(argv[0]);
            relative_set = true;
            arg_flag = NONE;
        }
        else if (arg_flag == SmoothCv) {
            char *end = nullptr;
            const double v = strtod(a.c_str(), &end);
            if (*end != '\0' || !(v > 0.0) || !std::isfinite(v)) return print_usage(argv[0]);
            smooth_sigma0[smooth_cv_args++] = v;
            if (smooth_cv_args == 2) arg_flag = NONE;
        }
        else if (arg_flag == Smooth) {
            char *end = nullptr;
            const double v = strtod(a.c_str(), &end);
            if (*end != '\0' || !(v > 0.0) || !std::isfinite(v)) return print_usage(argv[0]);
            smooth_sigma[smooth_args++] = v;
            if (smooth_args == 2) arg_flag = NONE;
        }
        else if (arg_flag == FixCams || arg_flag == FixMarkers) {
            if (!parse_ids(a, arg_flag == FixCams ? fixed_cams : fixed_markers)) return print_usage(argv[0]);
            (arg_flag == FixCams ? fix_cams : fix_markers) = true;
            arg_flag = NONE;
        }
        else if (arg_flag == PriorPath) { prior_path = a; arg_flag = NONE; }
        else if (arg_flag == RelPath) { rel_path = a; arg_flag = NONE; }
        else if (arg_flag == RelKinds) {
            if (a != "cams" && a != "markers" && a != "both") return print_usage(argv[0]);
            rel_kinds = a == "cams" ? 1 : (a == "markers" ? 2 : 3);
            arg_flag = NONE;
        }
        else if (arg_flag == RelDeg || arg_flag == RelM) {
            char *end = nullptr;
            const double v = strtod(a.c_str(), &end);
            if (*end != '\0' || !(v > 0.0) || !std::isfinite(v)) return print_usage(argv[0]);
            (arg_flag == RelDeg ? rel_sigma_deg : rel_sigma_m) = v;
            arg_flag = NONE;
        }
        else if (arg_flag == PriorDeg || arg_flag == PriorM) {
            char *end = nullptr;
            const double v = strtod(a.c_str(), &end);
            if (*end != '\0' || !(v > 0.0) || !std::isfinite(v)) return print_usage(argv[0]);
            (arg_flag == PriorDeg ? prior_sigma_deg : prior_sigma_m) = v;
            arg_flag = NONE;
        }
        else if (arg_flag == Leverage) {
            char *end = nullptr;
            const double v = strtod(a.c_str(), &end);
            if (*end != '\0' || a.empty() || !(v >= 0.0) || !std::isfinite(v)) return print_usage(argv[0]);
            leverage_min = v;
            leverage_set = true;
            arg_flag = NONE;
        }
        else if (arg_flag == Loo || arg_flag == RejectLoo) {
            char *end = nullptr;
            const double v = strtod(a.c_str(), &end);
            if (*end != '\0' || a.empty() || !(v > 0.0) || !std::isfinite(v)) return print_usage(argv[0]);
            (arg_flag == Loo ? loo_f_max : reject_loo_f) = v;
            arg_flag = NONE;
        }
        else if (arg_flag == SmoothLoo || arg_flag == SmoothRejectLoo) {
            char *end = nullptr;
            const double v = strtod(a.c_str(), &end);
            if (*end != '\0' || a.empty() || !(v > 0.0) || !std::isfinite(v)) return print_usage(argv[0]);
            (arg_flag == SmoothLoo ? smooth_loo_f : smooth_reject_loo_f) = v;
            arg_flag = NONE;
        }
        else if (arg_flag == RejectK || arg_flag == RejectPx) {
            const double v = stod(a);
            if (!(v > 0.0) && !(arg_flag == RejectPx && v == 0.0)) return print_usage(argv[0]);
            (arg_flag == RejectK ? reject_k : reject_min_px) = v;
            arg_flag = NONE;
        }
        else if (arg_flag == Solver) {
            solver = a == "spcg" ? AAR_SOLVER_SPCG : a == "pcg" ? AAR_SOLVER_PCG : a == "auto" ? AAR_SOLVER_AUTO : a == "direct" ? AAR_SOLVER_DIRECT : -1;
            if (solver < 0) return print_usage(argv[0]);
            arg_flag = NONE;
        }
        else if (arg_flag == ExcludeCams) excluded_cams.insert(stoi(a));
        else if (arg_flag == Threshold) { threshold = stod(a); arg_flag = NONE; }
    }
    if (smooth && (!tracking_only || smooth_args != 2)) return print_usage(argv[0]);
    if (smooth_covariance && !smooth) return print_usage(argv[0]);
    if (leverage && !leverage_set) return print_usage(argv[0]);
    if ((loo && !(loo_f_max > 0.0)) || (reject_loo_on && !(reject_loo_f > 0.0))) return print_usage(argv[0]);
    if ((loo || reject_loo_on) && with_huber) return print_usage(argv[0]);   // (the Huber weights break the Gaussian model the statistic rests on)
    if (smooth_cv && (!smooth || smooth_cv_args != 2 || smooth_covariance || fit_sigmas || resample)) return print_usage(argv[0]);
    if (cv_covariance && (!smooth || !smooth_cv)) return print_usage(argv[0]);
    if (cv_fit_sigmas && (!smooth || !smooth_cv || live)) return print_usage(argv[0]);
    if (fit_sigmas && (!smooth || live)) return print_usage(argv[0]);
    if (resample && (!smooth || live || resample_n < 2)) return print_usage(argv[0]);
    if (cv_resample && (!smooth || !smooth_cv || live || resample || resample_n < 2)) return print_usage(argv[0]);
    if (relative_to && (!smooth || live || !relative_set)) return print_usage(argv[0]);
    if ((smooth_loo && !(smooth_loo_f > 0.0)) || (smooth_reject_loo && !(smooth_reject_loo_f > 0.0))) return print_usage(argv[0]);
    if ((smooth_loo || smooth_reject_loo) && (!smooth || live || with_huber)) return print_usage(argv[0]);
    if (live && (!tracking_only || smooth || (live_args != 1 && live_args != 3) || (live_args == 1 && live_lag != 0))) return print_usage(argv[0]);
    if ((live_anchor_set || live_covariance) && (!live || arg_flag == Anchor)) return print_usage(argv[0]);
    if (live_anchor == AAR_TRACKER_ANCHOR_MARGINAL && (live_args != 3 || live_lag < 1)) return print_usage(argv[0]);
    if (live_gate && (!live || gate_args != 2 || (gate_v[0] <= 0.0 && gate_v[1] <= 0.0))) return print_usage(argv[0]);
    if (live_motion && (!live || motion_args < 1 || (motion_model == AAR_TRACKER_MOTION_CONSTANT_VELOCITY && live_args != 3))) return print_usage(argv[0]);
    if (from_detections && (!live || from_initial || use_subseqs || !excluded_cams.empty())) return print_usage(argv[0]);
    string name = "";
    if (tracking_only) name += "_tracking_only";
    if (use_subseqs) name += "_subseqs";
    if (with_huber) name += "_with_huber";
    if (!excluded_cams.empty()) {
        name += "_excluded_cams";
        for (int c : excluded_cams) name += "_" + to_string(c);
    }
    if (set_threshold) {
        char dbuf[32];
        snprintf(dbuf, sizeof dbuf, "%.1f", threshold);
        name += "_thresh_" + string(dbuf);
    }
    name += ".solution";
    const string initial_path = folder_path + "/initial" + name, final_path = folder_path + "/final" + name;

    // Initializer (apps/find_solution.cpp:101-113,142-147).  `-thresh` only names the files in the reference (the value never
    // reaches the Initializer, whose threshold stays 2.0, libs/initializer.h:52); kept that way.
    aar_cam_model *cams = nullptr;
    int32_t n_cams = 0;
    if (!from_initial && aar_cam_configs_read(folder_path.c_str(), &cams, &n_cams) != AAR_OK) n_cams = 0;
    const vector<aar_cam_model> cam_models(cams, cams + n_cams);
    if (from_detections && n_cams == 0) {
        cerr << "-from-detections: no calibration folders under " << folder_path << endl;
        return 1;
    }
    aar_dataset *init = nullptr;
    if (!from_initial && !from_detections && n_cams > 0) {
        try {
            vector<int> subseqs;
            if (use_subseqs) {
                int32_t *ss = nullptr, n_sub = 0;
                if (aar_subseqs_read((folder_path + "/subseqs.txt").c_str(), &ss, &n_sub)) throw runtime_error(aar_last_error());
                subseqs.assign(ss, ss + n_sub);
                free(ss);
            }
            aar_detections *detections = aar::Initializer::read_detections_file(folder_path + "/aruco.detections", subseqs);
            const long long n_det = detections->num_det;
            const auto t0 = chrono::system_clock::now();
            try {
                aar::Initializer initializer(detections, marker_size, vector<aar_cam_model>(cams, cams + n_cams), excluded_cams);
                init = initializer.release();
            } catch (...) {
                aar_detections_free(detections);
                throw;
            }
            aar_detections_free(detections);
            const chrono::duration<double> di = chrono::system_clock::now() - t0;
            cout << "Initializer: " << n_det << " detections -> " << init->num_cams << " cameras, " << init->num_markers << " markers, "
                 << init->num_frames << " frames in " << di.count() << " s" << endl;
        } catch (const exception &e) {
            cerr << "Initializer failed: " << e.what() << endl;
            free(cams);
            return 1;
        }
    }
    free(cams);
    aar::MultiCamMapper mcm(init);
    if (init) {
        mcm.write_solution_file(initial_path);
        mcm.write_text_solution_file(initial_path + ".yaml");
    } else if (!mcm.read_solution_file(initial_path)) {
        cerr << "No calibration folders under " << folder_path << " and no " << initial_path << endl;
        return 1;
    }
    if (fabs(mcm.get_marker_size() - (double)(float)marker_size) > 1e-9)
        cerr << "warning: marker_size argument " << marker_size << " differs from the solution file's " << mcm.get_marker_size() << endl;
    mcm.solver_params.verbose = true;
    mcm.set_optmize_flag_cam_intrinsics(false);  // apps/find_solution.cpp:140
    if (with_huber) mcm.set_with_huber(true);
    {
        aar::MultiCamMapper::SolverOptions so;
        so.solver = solver;
        mcm.set_solver_options(so);
    }
    const bool constrained = fix_cams || fix_markers || !prior_path.empty() || !rel_path.empty();
    if (constrained) {
        if (fix_cams) mcm.set_fixed_cams(fixed_cams);
        if (fix_markers) mcm.set_fixed_markers(fixed_markers);
        if (!prior_path.empty()) {
            vector<aar::MultiCamMapper::PosePrior> priors;
            if (read_pose_priors(prior_path, mcm.dataset(), prior_sigma_deg, prior_sigma_m, priors)) return 5;
            mcm.set_pose_priors(priors);
        }
        if (!rel_path.empty()) {
            vector<aar::MultiCamMapper::RelativePrior> rel;
            if (read_relative_priors(rel_path, mcm.dataset(), rel_kinds, rel_sigma_deg, rel_sigma_m, rel)) return 5;
            mcm.set_relative_priors(rel);
        }
        try {
            const aar::MultiCamMapper::ConstraintIndices k = mcm.constraint_indices();
            cout << "constraints: " << k.fixed_cams.size() << " fixed camera(s), " << k.fixed_markers.size() << " fixed marker(s), " << k.priors.size()
                 << " pose prior(s)";
            if (!prior_path.empty()) cout << " from " << prior_path << " (sigma " << prior_sigma_deg << " deg, " << prior_sigma_m << " m)";
            cout << endl;
            if (!rel_path.empty())
                cout << "constraints: " << k.pair_priors.size() << " relative pose prior(s) from " << rel_path << " (" << (rel_kinds == 1 ? "cams" : rel_kinds == 2 ? "markers" : "both")
                     << ", sigma " << rel_sigma_deg << " deg, " << rel_sigma_m << " m)" << endl;
        } catch (const exception &e) {
            cerr << "constraints: " << e.what() << endl;
            return 5;
        }
    }
    const auto start = chrono::system_clock::now();
    if (live) {
        aar::MultiCamMapper::LiveCovariance live_cov;
        aar::MultiCamMapper::LiveCovariance *want_cov = live_covariance ? &live_cov : nullptr;
        aar_tracker_gate_params gate_params;
        aar_tracker_default_gate_params(&gate_params);
        gate_params.k_median = gate_v[0];
        gate_params.min_px = gate_v[1];
        const aar_tracker_gate_params *want_gate = live_gate ? &gate_params : nullptr;
        aar_tracker_motion_params motion_params;
        aar_tracker_default_motion_params(&motion_params);
        motion_params.model = motion_model;
        motion_params.max_dt = motion_max_dt;
        const aar_tracker_motion_params *want_motion = live_motion ? &motion_params : nullptr;
        try {
            if (from_detections) {
                aar_detections *detections = aar::Initializer::read_detections_file(folder_path + "/aruco.detections", vector<int>());
                try {
                    mcm.track_live_from_detections(detections, cam_models, live_lag, live_args == 3, live_sigma[0], live_sigma[1], start_policy, live_anchor, want_cov, want_gate, want_motion);
                } catch (...) {
                    aar_detections_free(detections);
                    throw;
                }
                aar_detections_free(detections);
            } else {
                mcm.track_live(live_lag, live_args == 3, live_sigma[0], live_sigma[1], live_anchor, want_cov, want_gate, want_motion);
            }
            long long its = 0, rej = 0;
            double sec = 0, cost = 0;
            for (const aar_tracker_result &r : mcm.live_results) { its += r.iterations; rej += r.rejected_tries; sec += r.seconds; cost += r.final_cost; }
            cout << "live: " << mcm.live_results.size() << " pushes, lag " << live_lag << ", " << its << " LM iterations (" << rej << " rejected tries), summed cost "
                 << cost << ", " << (mcm.live_results.empty() ? 0.0 : 1e6 * sec / mcm.live_results.size()) << " us per push" << endl;
            if (from_detections) {
                long long held = 0, won = 0;
                for (const aar_tracker_start_info &si : mcm.live_starts) { held += si.voted; won += si.start_source == 2; }
                cout << "votes: " << held << " held, " << won << " won (start policy " << (start_policy == AAR_TRACKER_START_BEST ? "best" : "vote") << ")" << endl;
            }
            if (!mcm.live_motions.empty()) {
                long long predicted = 0;
                for (const aar_tracker_motion_info &m : mcm.live_motions) predicted += m.predicted;
                cout << "motion: constant velocity, " << predicted << " of " << mcm.live_motions.size() << " pushes with an expected motion (max_dt " << motion_max_dt << ")" << endl;
            }
            if (live_gate) {
                long long rejected = 0, frames = 0, small = 0;
                for (const aar_tracker_gate_info &g : mcm.live_gates) { rejected += g.n_in - g.n_kept; frames += g.n_kept < g.n_in; small += !g.gated; }
                cout << "gate: " << rejected << " detections rejected in " << frames << " frames (k_median " << gate_v[0] << ", min_px " << gate_v[1] << "; "
                     << small << " frames below min_detections = " << gate_params.min_detections << " were not gated)" << endl;
            }
        } catch (const exception &e) {
            cerr << "live tracking failed: " << e.what() << endl;
            return 6;
        }
        mcm.write_solution_file(final_path);
        mcm.write_text_solution_file(final_path + ".yaml");
        if (live_covariance) {
            const string cov_path = final_path + ".covariance.yaml";
            if (!mcm.write_live_covariance_file(cov_path, live_cov)) {
                cerr << "live covariance: " << aar_last_error() << endl;
                return 6;
            }
            cout << "live covariance: " << live_cov.valid.size() << " lagged blocks (anchor " << (live_anchor == AAR_TRACKER_ANCHOR_MARGINAL ? "marginal" : "fixed")
                 << ") written to " << cov_path << endl;
        }
        return 0;
    }
    try {
        mcm.solve();
    } catch (const exception &e) {
        cerr << "solve failed: " << e.what() << endl;
        return 2;
    }
    if (reject_k > 0.0 && reject_outliers(mcm, folder_path + "/final.residuals.yaml", reject_k, reject_min_px)) return 4;
    else if (residuals && reject_k <= 0.0) {
        const string res_path = folder_path + "/final.residuals.yaml";
        try {
            const aar::MultiCamMapper::ResidualReport rr = mcm.residual_report(nullptr);
            if (!mcm.write_residuals_file(res_path, rr)) throw runtime_error(aar_last_error());
            cout << "residuals: " << rr.report.num_detections << " detections, RMSE " << rr.report.rmse << " px, median " << rr.report.median << " px, max "
                 << rr.report.max << " px, written to " << res_path << endl;
        } catch (const exception &e) {
            cerr << "residual report failed: " << e.what() << endl;
            return 4;
        }
    }
    if (reject_loo_on && reject_loo(mcm, reject_loo_f)) return 4;
    if (smooth) {
        try {
            mcm.track();
            if (fit_sigmas) {
                aar::MultiCamMapper::SmoothFit sf;
                mcm.fit_smooth_sigmas(smooth_sigma[0], smooth_sigma[1], sf);
                const aar_smooth_fit_report &fr = sf.report;
                const streamsize keep = cout.precision(10);
                cout << "smooth-fit: sigma_px " << fr.sigma_px << " sigma_rot " << fr.sigma_rot << " sigma_trans " << fr.sigma_trans << " sigma_rot_eff "
                     << fr.sigma_rot_eff << " sigma_trans_eff " << fr.sigma_trans_eff << " after " << fr.iterations << " EM iterations (exit " << fr.stop_code
                     << ", " << fr.lm_steps << " LM iterations) in " << fr.seconds << " s" << endl;
                cout.precision(keep);
                smooth_sigma[0] = fr.sigma_rot_eff;
                smooth_sigma[1] = fr.sigma_trans_eff;
            }
            if (cv_fit_sigmas) {
                aar::MultiCamMapper::SmoothFit sf;
                mcm.fit_smooth_sigmas(smooth_sigma[0], smooth_sigma[1], AAR_SMOOTH_MODEL_CONSTANT_VELOCITY, smooth_sigma0[0], smooth_sigma0[1], sf);
                const aar_smooth_fit_report &fr = sf.report;
                const streamsize keep = cout.precision(10);
                cout << "smooth-cv-fit: sigma_px " << fr.sigma_px << " sigma_rot " << fr.sigma_rot << " sigma_trans " << fr.sigma_trans << " sigma_rot_eff "
                     << fr.sigma_rot_eff << " sigma_trans_eff " << fr.sigma_trans_eff << " sigma_rot0_eff " << smooth_sigma0[0] / fr.sigma_px
                     << " sigma_trans0_eff " << smooth_sigma0[1] / fr.sigma_px << " after " << fr.iterations << " EM iterations (exit " << fr.stop_code
                     << ", " << fr.lm_steps << " LM iterations) in " << fr.seconds << " s" << endl;
                cout.precision(keep);
                smooth_sigma[0] = fr.sigma_rot_eff;
                smooth_sigma[1] = fr.sigma_trans_eff;
                smooth_sigma0[0] /= fr.sigma_px;
                smooth_sigma0[1] /= fr.sigma_px;
            }
            if (smooth_cv) mcm.track_smooth(smooth_sigma[0], smooth_sigma[1], AAR_SMOOTH_MODEL_CONSTANT_VELOCITY, smooth_sigma0[0], smooth_sigma0[1]);
            else mcm.track_smooth(smooth_sigma[0], smooth_sigma[1]);
            const aar_smooth_report &sr = mcm.smooth_report;
            cout << "smooth: " << (smooth_cv ? "constant velocity, " : "") << sr.iterations << " LM iterations (" << sr.rejected_tries << " rejected tries, exit " << sr.stop_code << "), cost " << sr.initial_cost
                 << " -> " << sr.final_cost << " (data " << sr.final_data_cost << ", prior " << sr.final_prior_cost << ") in " << sr.seconds << " s" << endl;
            const int model = smooth_cv ? AAR_SMOOTH_MODEL_CONSTANT_VELOCITY : AAR_SMOOTH_MODEL_RANDOM_WALK;
            if (smooth_reject_loo) {
                int64_t total = 0;
                for (int round = 1; round <= 3; round++) {
                    aar::MultiCamMapper::SmoothLoo lo;
                    const int64_t dropped = mcm.smooth_reject_loo(smooth_sigma[0], smooth_sigma[1], model, smooth_sigma0[0], smooth_sigma0[1], smooth_reject_loo_f, &lo);
                    cout << "smooth-reject-loo round " << round << ": largest F " << lo.report.max_f << ", " << dropped << " detections dropped" << endl;
                    if (dropped == 0) break;
                    total += dropped;
                    mcm.track_smooth(smooth_sigma[0], smooth_sigma[1], model, smooth_sigma0[0], smooth_sigma0[1]);
                }
                cout << "smooth-reject-loo: " << total << " detections dropped, " << mcm.dataset()->num_obs << " left, cost " << mcm.smooth_report.final_cost << endl;
            }
            if (smooth_loo) {
                const string lo_path = folder_path + "/final.smooth_loo.yaml";
                aar::MultiCamMapper::SmoothLoo lo;
                mcm.track_smooth_detection_loo(smooth_sigma[0], smooth_sigma[1], model, smooth_sigma0[0], smooth_sigma0[1], smooth_loo_f, lo);
                if (aar_smooth_loo_write_yaml(lo_path.c_str(), mcm.dataset(), lo.F.data(), lo.q.data(), lo.leverage.data(), nullptr, lo.status.data(),
                                              lo.keep.data(), &lo.report))
                    throw runtime_error(aar_last_error());
                cout << "smooth-loo: largest F " << lo.report.max_f << ", " << lo.report.rejected << " above " << smooth_loo_f << ", " << lo.report.undetermined
                     << " undetermined, sigma2 " << lo.report.sigma2 << ", written to " << lo_path << endl;
            }
        } catch (const exception &e) {
            cerr << "smoothing failed: " << e.what() << endl;
            return 6;
        }
        if (smooth_covariance || cv_covariance) {
            const string cov_path = folder_path + "/final.smooth_covariance.yaml";
            try {
                aar::MultiCamMapper::SmoothCovariance sc;
                if (cv_covariance) mcm.track_smooth_covariance(smooth_sigma[0], smooth_sigma[1], AAR_SMOOTH_MODEL_CONSTANT_VELOCITY, smooth_sigma0[0], smooth_sigma0[1], sc);
                else mcm.track_smooth_covariance(smooth_sigma[0], smooth_sigma[1], sc);
                const size_t F = sc.frame_cov.size() / 36;
                aar::MultiCamMapper::LiveCovariance lc;
                lc.frame_cov = sc.frame_cov;
                lc.sigma2.assign(F, sc.report.sigma2);
                lc.valid.assign(F, 1);
                if (!mcm.write_live_covariance_file(cov_path, lc)) throw runtime_error(aar_last_error());
                double lo = 0.0, hi = 0.0;   // 1-sigma translation: sqrt(sigma2 * trace of the translation block)
                for (size_t f = 0; f < F; f++) {
                    const double *c = &sc.frame_cov[36 * f];
                    const double v = sqrt(sc.report.sigma2 * (c[21] + c[28] + c[35]));
                    if (f == 0 || v < lo) lo = v;
                    if (f == 0 || v > hi) hi = v;
                }
                cout << "smooth-covariance: sigma2 " << sc.report.sigma2 << " (" << sc.report.num_residuals << " residuals, " << sc.report.num_vars
                     << " unknowns), 1-sigma translation largest " << hi << " m, smallest " << lo << " m, written to " << cov_path << endl;
            } catch (const exception &e) {
                cerr << "smooth covariance failed: " << e.what() << endl;
                return 6;
            }
        }
    }
    if (smooth && (resample || cv_resample)) {
        const string rs_path = folder_path + "/final.resampled.yaml";
        try {
            // every gap of frame ids cut into resample_n equal parts; entry k * resample_n is frame k itself
            const aar_dataset *ds = mcm.dataset();
            vector<double> times;
            for (int f = 0; f < ds->num_frames; f++) {
                const double ta = (double)ds->frame_ids[f];
                times.push_back(ta);
                if (f + 1 < ds->num_frames)
                    for (int k = 1; k < resample_n; k++) times.push_back(ta + ((double)ds->frame_ids[f + 1] - ta) * ((double)k / (double)resample_n));
            }
            aar::MultiCamMapper::SmoothQuery q;
            if (cv_resample)
                mcm.track_smooth_query(smooth_sigma[0], smooth_sigma[1], AAR_SMOOTH_MODEL_CONSTANT_VELOCITY, smooth_sigma0[0], smooth_sigma0[1], times, q);
            else
                mcm.track_smooth_query(smooth_sigma[0], smooth_sigma[1], times, q);
            FILE *fp = fopen(rs_path.c_str(), "w");
            if (!fp) throw runtime_error("cannot write " + rs_path);
            fprintf(fp, "%%YAML:1.0\n---\nsigma2: %.17g\nresample: %d\nresampled_poses:\n", q.report.sigma2, resample_n);
            for (size_t k = 0; k < times.size(); k++) {
                fprintf(fp, "   - { time: %.17g, segment:%d, pose: [", times[k], (int)q.segment[k]);
                for (int i = 0; i < 6; i++) fprintf(fp, "%s%.17g", i ? ", " : "", q.pose[6 * k + i]);
                fprintf(fp, "],\n       covariance: !!opencv-matrix { rows:6, cols:6, dt:d, data:[");
                for (int i = 0; i < 36; i++) fprintf(fp, "%s%.17g", i ? ", " : "", q.report.sigma2 * q.cov[36 * k + i]);
                fprintf(fp, "] } }\n");
            }
            fclose(fp);
            cout << "resample: " << times.size() << " poses (" << q.report.num_on_frame << " on frames, " << q.report.num_inside << " between), sigma2 "
                 << q.report.sigma2 << ", written to " << rs_path << endl;
        } catch (const exception &e) {
            cerr << "resampling failed: " << e.what() << endl;
            return 6;
        }
    }
    const chrono::duration<double> d = chrono::system_clock::now() - start;
    mcm.write_solution_file(final_path);
    mcm.write_text_solution_file(final_path + ".yaml");
    if (smooth && relative_to) {
        const string rl_path = folder_path + "/final.smooth_relative.yaml";
        try {
            // at the poses AS THE SOLUTION FILE HOLDS THEM (its writer stores Rodrigues(matrix) of every pose: a few ulps from the driver's own
            // vector), read back into a mapper of its own: the two files written side by side agree to the bit, and mcm stays as it is
            aar::MultiCamMapper at_file;
            if (!at_file.read_solution_file(final_path)) throw runtime_error("cannot read back " + final_path);
            at_file.set_optmize_flag_cam_intrinsics(false);
            if (with_huber) at_file.set_with_huber(true);
            const aar_dataset *ds = at_file.dataset();
            int base = -1;
            for (int f = 0; f < ds->num_frames; f++)
                if ((long)ds->frame_ids[f] == relative_id) base = f;
            if (base < 0) throw runtime_error("-relative-to: the recording has no frame with id " + to_string(relative_id));
            vector<pair<int32_t, int32_t>> pairs;
            for (int f = 0; f < ds->num_frames; f++) pairs.push_back({(int32_t)base, (int32_t)f});
            aar::MultiCamMapper::SmoothRelative q;
            at_file.track_smooth_relative(smooth_sigma[0], smooth_sigma[1], smooth_cv ? AAR_SMOOTH_MODEL_CONSTANT_VELOCITY : AAR_SMOOTH_MODEL_RANDOM_WALK,
                                      smooth_sigma0[0], smooth_sigma0[1], pairs, q);
            FILE *fp = fopen(rl_path.c_str(), "w");
            if (!fp) throw runtime_error("cannot write " + rl_path);
            fprintf(fp, "%%YAML:1.0\n---\nsigma2: %.17g\nrelative_to: %ld\nrelative_motions:\n", q.report.sigma2, relative_id);
            for (size_t k = 0; k < pairs.size(); k++) {
                fprintf(fp, "   - { frame: %d, baseline: %.17g, rel: [", (int)ds->frame_ids[k], (double)ds->frame_ids[k] - (double)ds->frame_ids[base]);
                for (int i = 0; i < 6; i++) fprintf(fp, "%s%.17g", i ? ", " : "", q.rel[6 * k + i]);
                fprintf(fp, "],\n       covariance: !!opencv-matrix { rows:6, cols:6, dt:d, data:[");
                for (int i = 0; i < 36; i++) fprintf(fp, "%s%.17g", i ? ", " : "", q.report.sigma2 * q.rel_cov[36 * k + i]);
                fprintf(fp, "] } }\n");
            }
            fclose(fp);
            cout << "smooth-relative: " << pairs.size() << " frames relative to frame " << relative_id << " (" << q.report.num_direct << " from the blocks, "
                 << q.report.num_chained << " chained, longest lag " << q.report.max_lag << "), sigma2 " << q.report.sigma2 << ", written to " << rl_path << endl;
        } catch (const exception &e) {
            cerr << "smooth relative failed: " << e.what() << endl;
            return 6;
        }
    }
    if (covariance) {
        const string cov_path = folder_path + "/final.covariance.yaml";
        try {
            const aar::MultiCamMapper::Covariance cv = mcm.compute_covariance(true);
            if (!mcm.write_covariance_file(cov_path, cv)) throw runtime_error(aar_last_error());
            cout << "covariance: sigma2 " << cv.sigma2 << " (" << cv.report.num_residuals << " residuals, " << cv.report.num_vars << " unknowns), written to "
                 << cov_path << endl;
        } catch (const exception &e) {
            cerr << "covariance failed: " << e.what() << endl;
            return 3;
        }
    }
    if (leverage) {
        const string lev_path = folder_path + "/final.leverage.yaml";
        try {
            const aar::MultiCamMapper::DetectionLeverage lv = mcm.detection_leverage(false);
            const aar::MultiCamMapper::ResidualReport rr = mcm.residual_report(nullptr);
            if (!mcm.write_leverage_file(lev_path, lv, leverage_min, rr.det_err)) throw runtime_error(aar_last_error());
            int64_t listed = 0;
            for (double h : lv.leverage) listed += !(h < leverage_min);
            cout << "leverage: sum " << lv.report.leverage_sum << " over " << lv.leverage.size() << " detections (" << lv.report.num_live_vars
                 << " live unknowns), " << listed << " at " << leverage_min << " or above, written to " << lev_path << endl;
        } catch (const exception &e) {
            cerr << "leverage failed: " << e.what() << endl;
            return 3;
        }
    }
    if (loo) {
        const string loo_path = folder_path + "/final.loo.yaml";
        try {
            const aar::MultiCamMapper::DetectionLoo lo = mcm.detection_loo(loo_f_max);
            const aar::MultiCamMapper::ResidualReport rr = mcm.residual_report(nullptr);
            if (!mcm.write_loo_file(loo_path, lo, rr.det_err)) throw runtime_error(aar_last_error());
            cout << "leave-one-out: largest F " << lo.report.max_f << ", " << lo.report.rejected << " above " << loo_f_max << ", " << lo.report.undetermined
                 << " undetermined of " << lo.F.size() << " detections, written to " << loo_path << endl;
        } catch (const exception &e) {
            cerr << "leave-one-out failed: " << e.what() << endl;
            return 3;
        }
    }
    const aar_lm_report &r = mcm.last_report;
    {
        const aar_solver_stats st = mcm.solver_stats();
        const char *names[] = {"direct", "pcg", "spcg", "auto"};
        cout << "solver: " << names[st.solver & 3] << ", " << st.total_iterations << " CG iterations in " << st.solves << " damped solves, " << st.fallbacks
             << " redone by the direct chain" << endl;
    }
    cout << "LM iterations: " << r.iterations << "  error " << r.initial_err << " -> " << r.final_err << "  (" << r.iterations / r.solve_seconds
         << " LM it/s in the solver loop)" << endl;
    if (constrained) {
        try {
            const double pc = mcm.prior_cost(), rc_ = rel_path.empty() ? 0.0 : mcm.relative_prior_cost();
            cout << "final error: reprojection " << r.final_err - pc - rc_ << " + prior " << pc;
            if (!rel_path.empty()) cout << " + relative prior " << rc_;
            cout << endl;
        } catch (const exception &e) {
            cerr << "prior cost failed: " << e.what() << endl;
            return 3;
        }
    }
    const int minutes = (int)(d.count() / 60);
    const int seconds = (int)lround(d.count() - minutes * 60);
    cout << "The algorithm took: " << minutes << " minutes " << seconds << " seconds" << endl;
    return 0;
}
