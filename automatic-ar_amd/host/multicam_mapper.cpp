// MultiCamMapper over the C ABI (see multicam_mapper.h).  Only packing / unpacking of parameter
// vectors and file I/O happen on the host; residuals, Jacobians and the LM solve are HIP kernels.
#include "multicam_mapper.h"

#include <algorithm>
#include <cstdio>
#include <cstring>
#include <functional>
#include <iostream>
#include <stdexcept>
#include <string>

#include "internal.h"
#include "se3.h"

namespace aar {

MultiCamMapper::MultiCamMapper() {
    solver_params.maxIters = 10000;  // libs/multicam_mapper.cpp:337-343
    solver_params.min_average_step_error_diff = 1e-4;
    memset(&last_report, 0, sizeof last_report);
}

MultiCamMapper::MultiCamMapper(aar_dataset *dataset) : MultiCamMapper() {
    data_ = dataset;
    solver_params.verbose = true;  // :327
    if (data_) {
        config_.optimize_cam_poses = data_->optimize_cam_poses != 0;
        config_.optimize_marker_poses = data_->optimize_marker_poses != 0;
        config_.optimize_object_poses = data_->optimize_object_poses != 0;
        config_.optimize_cam_intrinsics = data_->optimize_cam_intrinsics != 0;
        mats2eVec();
    }
}

MultiCamMapper::MultiCamMapper(Initializer &initializer) : MultiCamMapper(initializer.release()) {}

static Rigid from44(const Mat44 &m) {
    Rigid T;
    for (int r = 0; r < 3; r++) {
        for (int c = 0; c < 3; c++) T.R[r * 3 + c] = m[r * 4 + c];
        T.t[r] = m[r * 4 + 3];
    }
    return T;
}

MultiCamMapper::MultiCamMapper(size_t root_c, const std::map<int, Mat44> &T_to_root_cam, size_t root_m, const std::map<int, Mat44> &T_to_root_marker,
                               const std::map<int, Mat44> &obj_transforms, const FrameCamMarkers &fcm, float m_size,
                               std::vector<aar_cam_model> &cam_confs)
    : MultiCamMapper() {
    init(root_c, T_to_root_cam, root_m, T_to_root_marker, obj_transforms, fcm, m_size, cam_confs);
}

// frames (ascending id), their poses, and the detections in the reference's residual order -- frame, camera, detection order
// (libs/multicam_mapper.cpp:1001-1007) -- minus what fill_iteration_arrays erases: cameras / markers without a transform (:356-367)
void MultiCamMapper::load_frames(const std::map<int, Mat44> &object_poses, const FrameCamMarkers &fcm) {
    aar_dataset *old = data_;
    std::map<int, int> cam_index, marker_index, frame_index;
    for (int c = 0; c < old->num_cams; c++) cam_index[old->cam_ids[c]] = c;
    for (int m = 0; m < old->num_markers; m++) marker_index[old->marker_ids[m]] = m;
    int fi = 0;
    for (const auto &kv : object_poses) frame_index[kv.first] = fi++;
    struct O { int f, c, m; const float *uv; };
    std::vector<O> obs;
    for (const auto &fr : fcm) {
        auto f = frame_index.find(fr.first);
        if (f == frame_index.end()) throw std::runtime_error("MultiCamMapper::init: detections of frame " + std::to_string(fr.first) + " without an object pose");   // the reference: std::map::at
        for (const auto &cm : fr.second) {
            auto c = cam_index.find(cm.first);
            if (c == cam_index.end()) continue;
            for (const Marker &mk : cm.second) {
                auto m = marker_index.find(mk.id);
                if (m == marker_index.end()) continue;
                obs.push_back({f->second, c->second, m->second, mk.corners});
            }
        }
    }
    const int C = old->num_cams, M = old->num_markers, F = (int)object_poses.size();
    aar_dataset *d = dataset_alloc(C, M, F, (int64_t)obs.size(), false);
    memcpy(d->cam_ids, old->cam_ids, sizeof(int32_t) * C);
    memcpy(d->marker_ids, old->marker_ids, sizeof(int32_t) * M);
    memcpy(d->image_sizes, old->image_sizes, sizeof(int32_t) * 2 * C);
    memcpy(d->cam_mats, old->cam_mats, sizeof(double) * 9 * C);
    memcpy(d->dist_coeffs, old->dist_coeffs, sizeof(double) * 5 * C);
    d->root_cam = old->root_cam; d->root_marker = old->root_marker; d->marker_size = old->marker_size;
    d->optimize_cam_poses = old->optimize_cam_poses; d->optimize_marker_poses = old->optimize_marker_poses;
    d->optimize_object_poses = old->optimize_object_poses; d->optimize_cam_intrinsics = old->optimize_cam_intrinsics;
    const int64_t shared = 6LL * (C - 1) + 6LL * (M - 1);
    memcpy(d->x_full, old->x_full, sizeof(double) * shared);
    fi = 0;
    for (const auto &kv : object_poses) {
        d->frame_ids[fi] = kv.first;
        rigid_to_pose(from44(kv.second), d->x_full + shared + 6LL * fi);
        fi++;
    }
    for (size_t i = 0; i < obs.size(); i++) {
        d->obs_frame[i] = obs[i].f; d->obs_cam[i] = obs[i].c; d->obs_marker[i] = obs[i].m;
        memcpy(d->obs_uv + 8 * i, obs[i].uv, sizeof(float) * 8);
    }
    drop_problem();
    aar_dataset_free(old);
    data_ = d;
    remove_distortions();
    mats2eVec();
}

void MultiCamMapper::init(const std::map<int, Mat44> &object_poses, const FrameCamMarkers &fcm) {   // libs/multicam_mapper.cpp:272-279
    if (!data_) throw std::runtime_error("MultiCamMapper::init(object_poses, fcm): the mapper holds no cameras / markers yet");
    load_frames(object_poses, fcm);
}

void MultiCamMapper::init(size_t root_c, const std::map<int, Mat44> &T_to_root_cam, size_t root_m, const std::map<int, Mat44> &T_to_root_marker,
                          const std::map<int, Mat44> &object_poses, const FrameCamMarkers &fcm, float m_size,
                          const std::vector<aar_cam_model> &cam_confs) {   // libs/multicam_mapper.cpp:281-335
    if (T_to_root_cam.empty() || T_to_root_marker.empty()) throw std::runtime_error("MultiCamMapper::init: no cameras / markers");
    if (!T_to_root_cam.count((int)root_c) || !T_to_root_marker.count((int)root_m)) throw std::runtime_error("MultiCamMapper::init: root id without a transform");
    const int C = (int)T_to_root_cam.size(), M = (int)T_to_root_marker.size();
    aar_dataset *d = dataset_alloc(C, M, 0, 0, false);
    cam_models_.assign(C, aar_cam_model());
    int i = 0;
    for (const auto &kv : T_to_root_cam) {   // ascending id = MatArray order (libs/multicam_mapper.h:95-105)
        const int id = kv.first;
        if (id < 0 || id >= (int)cam_confs.size()) { aar_dataset_free(d); throw std::runtime_error("MultiCamMapper::init: no calibration for camera id " + std::to_string(id)); }   // cam_configs[cam_id], :314
        d->cam_ids[i] = id;
        if (id == (int)root_c) d->root_cam = i;
        const aar_cam_model &cc = cam_confs[id];
        memcpy(d->cam_mats + 9 * i, cc.K, sizeof cc.K);
        for (int j = 0; j < 5; j++) d->dist_coeffs[5 * i + j] = cc.dist[j];
        d->image_sizes[2 * i] = cc.width; d->image_sizes[2 * i + 1] = cc.height;
        cam_models_[i] = cc;
        i++;
    }
    i = 0;
    for (const auto &kv : T_to_root_marker) {
        d->marker_ids[i] = kv.first;
        if (kv.first == (int)root_m) d->root_marker = i;
        i++;
    }
    PoseLayout L;
    L.C = C; L.M = M; L.F = 0; L.rc = d->root_cam; L.rm = d->root_marker;
    i = 0;
    for (const auto &kv : T_to_root_cam) { if (i != L.rc) rigid_to_pose(from44(kv.second), d->x_full + L.full_cam0() + 6LL * L.cam_slot(i)); i++; }
    i = 0;
    for (const auto &kv : T_to_root_marker) { if (i != L.rm) rigid_to_pose(from44(kv.second), d->x_full + L.full_mk0() + 6LL * L.mk_slot(i)); i++; }
    d->marker_size = (double)m_size;   // float parameter, libs/multicam_mapper.h:20
    d->optimize_cam_intrinsics = 1;    // a fresh mapper holds the default Config (libs/multicam_mapper.h:75-81)
    drop_problem();
    aar_dataset_free(data_);
    data_ = d;
    config_ = Config();
    solver_params = SparseLevMarq<double>::Params();   // :326-330
    solver_params.verbose = true;
    solver_params.maxIters = 10000;
    solver_params.min_average_step_error_diff = 1e-4;
    load_frames(object_poses, fcm);
    // eval_curr_solution + "the very initial error" (:331-333); the pose groups only, as error_function evaluates them
    const Config keep = config_;
    config_.optimize_cam_intrinsics = false;
    drop_problem();
    if (ensure_problem()) { config_ = keep; throw std::runtime_error(aar_last_error()); }
    double e0 = 0;
    const int rc = aar_eval_residuals(problem_, data_->x_full, nullptr, &e0);
    config_ = keep;
    drop_problem();   // (built for the pose groups only)
    if (rc) throw std::runtime_error(aar_last_error());
    std::cout << "the very initial error: " << e0 << std::endl;
}

MultiCamMapper::~MultiCamMapper() {
    drop_problem();
    aar_dataset_free(data_);
}

void MultiCamMapper::drop_problem() {
    solver.detach();   // the solver keeps the raw handle between init() / step() calls: never let it outlive the problem
    if (problem_) aar_problem_destroy(problem_);
    problem_ = nullptr;
}

namespace detail {
EvalProbe &eval_probe() {
    static thread_local EvalProbe p;
    return p;
}
aar_problem *current_problem(const MultiCamMapper *owner) { return owner ? owner->problem_ : nullptr; }
aar_problem *bind_problem(MultiCamMapper *owner, std::vector<double> &x_full) {
    if (!owner || !owner->data_) throw std::runtime_error("SparseLevMarq: the evaluation functions belong to a MultiCamMapper without a data set");
    if (owner->ensure_problem()) throw std::runtime_error(aar_last_error());
    if (owner->with_huber_ && aar_problem_set_huber_delta(owner->problem_, owner->hubberDelta)) throw std::runtime_error(aar_last_error());
    x_full = owner->problem_vector();
    return owner->problem_;
}
}  // namespace detail

bool MultiCamMapper::probed(int kind) {
    detail::EvalProbe &p = detail::eval_probe();
    if (!p.active) return false;
    p.id.owner = this;
    p.id.kind = kind;
    return true;
}

void MultiCamMapper::set_optmize_flag_cam_poses(bool f) { config_.optimize_cam_poses = f; drop_problem(); }
void MultiCamMapper::set_optmize_flag_marker_poses(bool f) { config_.optimize_marker_poses = f; drop_problem(); }
void MultiCamMapper::set_optmize_flag_object_poses(bool f) { config_.optimize_object_poses = f; drop_problem(); }
void MultiCamMapper::set_optmize_flag_cam_intrinsics(bool f) { config_.optimize_cam_intrinsics = f; drop_problem(); }
void MultiCamMapper::set_with_huber(bool wh) { with_huber_ = wh; drop_problem(); }
void MultiCamMapper::set_config(Config &conf) { config_ = conf; drop_problem(); }

size_t MultiCamMapper::get_num_vars(const Config &conf) {  // libs/multicam_mapper.cpp:239-250
    if (!data_) return 0;
    size_t n = 0;
    if (conf.optimize_cam_poses) n += (size_t)(data_->num_cams - 1) * 6;
    if (conf.optimize_marker_poses) n += (size_t)(data_->num_markers - 1) * 6;
    if (conf.optimize_object_poses) n += (size_t)data_->num_frames * 6;
    if (conf.optimize_cam_intrinsics) n += (size_t)data_->num_cams * 9;
    return n;
}

// mats2eVec (:445-461): the optimised groups of x_full, cameras | markers | frames | intrinsics
void MultiCamMapper::mats2eVec() {
    io_vec.assign(get_num_vars(config_), 0.0);
    if (!data_) return;
    PoseLayout L;
    L.C = data_->num_cams; L.M = data_->num_markers; L.F = data_->num_frames;
    size_t k = 0;
    auto copy = [&](int64_t off, int64_t n) { for (int64_t i = 0; i < n; i++) io_vec[k++] = data_->x_full[off + i]; };
    if (config_.optimize_cam_poses) copy(L.full_cam0(), 6LL * (L.C - 1));
    if (config_.optimize_marker_poses) copy(L.full_mk0(), 6LL * (L.M - 1));
    if (config_.optimize_object_poses) copy(L.full_fr0(), 6LL * L.F);
    if (config_.optimize_cam_intrinsics)
        for (int c = 0; c < L.C; c++) {  // fill_io_vec_cam_intrinsics, :488-498
            const double *K = data_->cam_mats + 9 * c;
            io_vec[k++] = K[0]; io_vec[k++] = K[2]; io_vec[k++] = K[4]; io_vec[k++] = K[5];
            for (int j = 0; j < 5; j++) io_vec[k++] = data_->dist_coeffs[5 * c + j];
        }
}

// eVec2Mats (:595-606)
void MultiCamMapper::eVec2Mats(const eVector &v) {
    PoseLayout L;
    L.C = data_->num_cams; L.M = data_->num_markers; L.F = data_->num_frames;
    size_t k = 0;
    auto copy = [&](int64_t off, int64_t n) { for (int64_t i = 0; i < n; i++) data_->x_full[off + i] = v[k++]; };
    if (config_.optimize_cam_poses) copy(L.full_cam0(), 6LL * (L.C - 1));
    if (config_.optimize_marker_poses) copy(L.full_mk0(), 6LL * (L.M - 1));
    if (config_.optimize_object_poses) copy(L.full_fr0(), 6LL * L.F);
    if (config_.optimize_cam_intrinsics)
        for (int c = 0; c < L.C; c++) {  // intrinsics_vec2mats, :580-593: cv::Mat::eye with fx, cx, fy, cy (a skew is gone), then d0..d4
            double *K = data_->cam_mats + 9 * c;
            K[0] = v[k++]; K[1] = 0; K[2] = v[k++]; K[3] = 0; K[4] = v[k++]; K[5] = v[k++]; K[6] = 0; K[7] = 0; K[8] = 1;
            for (int j = 0; j < 5; j++) data_->dist_coeffs[5 * c + j] = v[k++];
        }
}

// x_full of the device problem for the current Config: the pose vector, followed -- with optimize_cam_intrinsics -- by
// fx cx fy cy d0..d4 per camera (fill_io_vec_cam_intrinsics, :488-498), i.e. the `.solution` vector
std::vector<double> MultiCamMapper::problem_vector() {
    std::vector<double> x(data_->x_full, data_->x_full + aar_dataset_full_len(data_));
    if (config_.optimize_cam_intrinsics)
        for (int c = 0; c < data_->num_cams; c++) {
            const double *K = data_->cam_mats + 9 * c;
            x.push_back(K[0]); x.push_back(K[2]); x.push_back(K[4]); x.push_back(K[5]);
            for (int j = 0; j < 5; j++) x.push_back(data_->dist_coeffs[5 * c + j]);
        }
    return x;
}

int MultiCamMapper::ensure_problem() {
    if (problem_) return AAR_OK;
    aar_problem_desc d;
    aar_problem_desc_from_dataset(data_, &d);
    d.optimize_cam_poses = config_.optimize_cam_poses;
    d.optimize_marker_poses = config_.optimize_marker_poses;
    d.optimize_object_poses = config_.optimize_object_poses;
    d.optimize_cam_intrinsics = config_.optimize_cam_intrinsics;
    d.residual_mode = residual_mode;
    d.with_huber = with_huber_ ? 1 : 0;
    d.device_id = device_id;
    aar_solver_options so;
    aar_solver_default_options(&so);
    so.solver = solver_options_.solver;
    so.deterministic = solver_options_.deterministic ? 1 : 0;
    so.pcg_eta = solver_options_.pcg_eta;
    so.pcg_max_it = solver_options_.pcg_max_it;
    so.pcg_eta_loose = solver_options_.pcg_eta_loose;
    so.pcg_eta_switch = solver_options_.pcg_eta_switch;
    so.pcg_abs_tol = solver_options_.pcg_abs_tol;
    const ConstraintIndices k = constraint_indices();
    int rc;
    if (k.empty()) {
        rc = aar_problem_create_ex(&d, &so, &problem_);
    } else {
        aar_problem_constraints c;
        memset(&c, 0, sizeof c);
        c.struct_size = (uint32_t)sizeof c;
        c.n_fixed_cams = (int32_t)k.fixed_cams.size(); c.fixed_cams = k.fixed_cams.data();
        c.n_fixed_markers = (int32_t)k.fixed_markers.size(); c.fixed_markers = k.fixed_markers.data();
        c.n_priors = (int32_t)k.priors.size(); c.priors = k.priors.data();
        c.n_pair_priors = (int32_t)k.pair_priors.size(); c.pair_priors = k.pair_priors.data();
        rc = aar_problem_create_constrained(&d, &so, &c, &problem_);
    }
    if (!rc && with_huber_) rc = aar_problem_set_huber_delta(problem_, hubberDelta);
    return rc;
}

void MultiCamMapper::set_fixed_cams(std::set<int> ids) { fixed_cam_ids_ = std::move(ids); drop_problem(); }
void MultiCamMapper::set_fixed_markers(std::set<int> ids) { fixed_marker_ids_ = std::move(ids); drop_problem(); }
void MultiCamMapper::set_pose_priors(std::vector<PosePrior> priors) { pose_priors_ = std::move(priors); drop_problem(); }
void MultiCamMapper::set_relative_priors(std::vector<RelativePrior> priors) { relative_priors_ = std::move(priors); drop_problem(); }

MultiCamMapper::ConstraintIndices MultiCamMapper::constraint_indices() const {
    ConstraintIndices k;
    if (!data_) return k;
    auto index_of = [](const int32_t *ids, int n, int id, const char *what) -> int {
        const int32_t *e = ids + n, *p = std::lower_bound(ids, e, id);   // (ids ascending)
        if (p == e || *p != id) throw std::invalid_argument(std::string("MultiCamMapper: no ") + what + " with id " + std::to_string(id));
        return (int)(p - ids);
    };
    const int C = data_->num_cams, M = data_->num_markers;
    std::vector<uint8_t> held(C + M, 0);
    for (int c = 0; c < C; c++) held[c] = (c == data_->root_cam || !config_.optimize_cam_poses) ? 1 : 0;
    for (int m = 0; m < M; m++) held[C + m] = (m == data_->root_marker || !config_.optimize_marker_poses) ? 1 : 0;
    for (int id : fixed_cam_ids_) { const int c = index_of(data_->cam_ids, C, id, "camera"); k.fixed_cams.push_back(c); held[c] = 1; }
    for (int id : fixed_marker_ids_) { const int m = index_of(data_->marker_ids, M, id, "marker"); k.fixed_markers.push_back(m); held[C + m] = 1; }
    for (const PosePrior &q : pose_priors_) {
        aar_pose_prior p;
        memset(&p, 0, sizeof p);
        p.kind = q.kind;
        p.index = q.kind == AAR_PRIOR_CAMERA ? index_of(data_->cam_ids, C, q.id, "camera") : index_of(data_->marker_ids, M, q.id, "marker");
        if (held[q.kind == AAR_PRIOR_CAMERA ? p.index : C + p.index]) continue;
        rigid_to_pose(from44(q.T), p.x6);
        memcpy(p.info, q.info.data(), sizeof p.info);
        k.priors.push_back(p);
    }
    for (const RelativePrior &q : relative_priors_) {
        aar_pair_prior p;
        memset(&p, 0, sizeof p);
        p.kind = q.kind;
        const bool cam = q.kind == AAR_PRIOR_CAMERA;
        p.index_a = cam ? index_of(data_->cam_ids, C, q.id_a, "camera") : index_of(data_->marker_ids, M, q.id_a, "marker");
        p.index_b = cam ? index_of(data_->cam_ids, C, q.id_b, "camera") : index_of(data_->marker_ids, M, q.id_b, "marker");
        if (held[cam ? p.index_a : C + p.index_a] && held[cam ? p.index_b : C + p.index_b]) continue;
        rigid_to_pose(from44(q.T), p.x6_rel);
        memcpy(p.info, q.info.data(), sizeof p.info);
        k.pair_priors.push_back(p);
    }
    return k;
}

double MultiCamMapper::relative_prior_cost() {
    if (!data_) throw std::runtime_error("MultiCamMapper::relative_prior_cost: no data set");
    if (ensure_problem()) throw std::runtime_error(aar_last_error());
    if (aar_problem_num_pair_priors(problem_) == 0) return 0.0;
    std::vector<double> x = problem_vector();
    double cost = 0;
    if (aar_problem_eval_pair_priors(problem_, x.data(), nullptr, &cost)) throw std::runtime_error(aar_last_error());
    return cost;
}

double MultiCamMapper::prior_cost() {
    if (!data_) throw std::runtime_error("MultiCamMapper::prior_cost: no data set");
    if (ensure_problem()) throw std::runtime_error(aar_last_error());
    if (aar_problem_num_priors(problem_) == 0) return 0.0;
    std::vector<double> x = problem_vector();
    double cost = 0;
    if (aar_problem_eval_priors(problem_, x.data(), nullptr, &cost)) throw std::runtime_error(aar_last_error());
    return cost;
}

void MultiCamMapper::set_solver_options(const SolverOptions &o) {
    solver_options_ = o;
    drop_problem();   // (the solver is a property of the device problem: the next solve() / track() builds one with these options)
}

aar_solver_stats MultiCamMapper::solver_stats() {
    if (!data_) throw std::runtime_error("MultiCamMapper::solver_stats: no data set");
    if (ensure_problem()) throw std::runtime_error(aar_last_error());
    aar_solver_stats st;
    st.struct_size = (uint32_t)sizeof st;
    if (aar_problem_get_solver_stats(problem_, &st)) throw std::runtime_error(aar_last_error());
    return st;
}

MultiCamMapper::Covariance MultiCamMapper::compute_covariance(bool frames) {
    if (!data_) throw std::runtime_error("MultiCamMapper::compute_covariance: no data set");
    if (ensure_problem()) throw std::runtime_error(aar_last_error());
    const int C = data_->num_cams, M = data_->num_markers, F = data_->num_frames;
    const size_t n_diag = 36 * (size_t)((config_.optimize_cam_poses ? C - 1 : 0) + (config_.optimize_marker_poses ? M - 1 : 0)) +
                          (config_.optimize_cam_intrinsics ? 81 * (size_t)C : 0);
    Covariance cv;
    cv.entity_diag.assign(std::max<size_t>(n_diag, 1), NAN);
    frames = frames && config_.optimize_object_poses;
    if (frames) cv.frame_cov.assign(36 * (size_t)F, NAN);
    cv.report.struct_size = (uint32_t)sizeof cv.report;
    std::vector<double> x = problem_vector();
    if (aar_problem_covariance(problem_, x.data(), nullptr, cv.entity_diag.data(), frames ? cv.frame_cov.data() : nullptr, &cv.report))
        throw std::runtime_error(aar_last_error());
    cv.sigma2 = cv.report.sigma2;
    auto scaled = [&](const double *b) { Mat66 m; for (int k = 0; k < 36; k++) m[k] = b ? cv.sigma2 * b[k] : NAN; return m; };
    const size_t mk0 = config_.optimize_cam_poses ? 36 * (size_t)(C - 1) : 0;
    for (int c = 0; c < C; c++) {
        const int s = c == data_->root_cam ? -1 : (c < data_->root_cam ? c : c - 1);
        cv.cams[data_->cam_ids[c]] = scaled((s < 0 || !config_.optimize_cam_poses) ? nullptr : cv.entity_diag.data() + 36 * (size_t)s);
    }
    for (int m = 0; m < M; m++) {
        const int s = m == data_->root_marker ? -1 : (m < data_->root_marker ? m : m - 1);
        cv.markers[data_->marker_ids[m]] = scaled((s < 0 || !config_.optimize_marker_poses) ? nullptr : cv.entity_diag.data() + mk0 + 36 * (size_t)s);
    }
    if (frames)
        for (int f = 0; f < F; f++) cv.objects[data_->frame_ids[f]] = scaled(cv.frame_cov.data() + 36 * (size_t)f);
    return cv;
}

bool MultiCamMapper::write_covariance_file(const std::string &path, const Covariance &cov) {
    if (!data_) return false;
    // (the writer reads the group flags from the data set: the mapper's Config is what the covariance was computed for)
    aar_dataset d = *data_;
    d.optimize_cam_poses = config_.optimize_cam_poses;
    d.optimize_marker_poses = config_.optimize_marker_poses;
    return aar_covariance_write_yaml(path.c_str(), &d, cov.entity_diag.data(), cov.frame_cov.empty() ? nullptr : cov.frame_cov.data(), cov.sigma2) == AAR_OK;
}

MultiCamMapper::ResidualReport MultiCamMapper::residual_report(const aar_outlier_rule *rule) {
    if (!data_) throw std::runtime_error("MultiCamMapper::residual_report: no data set");
    if (ensure_problem()) throw std::runtime_error(aar_last_error());
    ResidualReport rr;
    const size_t N = (size_t)data_->num_obs;
    rr.det_err.assign(std::max<size_t>(N, 1), 0.0);
    rr.keep.assign(std::max<size_t>(N, 1), 1);
    rr.cam_stats.assign(4 * (size_t)data_->num_cams, 0.0);
    rr.marker_stats.assign(4 * (size_t)data_->num_markers, 0.0);
    rr.frame_stats.assign(4 * (size_t)std::max(data_->num_frames, 1), 0.0);
    rr.report.struct_size = (uint32_t)sizeof rr.report;
    std::vector<double> x = problem_vector();
    if (aar_problem_residual_report(problem_, x.data(), rule, rr.det_err.data(), rr.keep.data(), rr.cam_stats.data(), rr.marker_stats.data(),
                                    rr.frame_stats.data(), &rr.report))
        throw std::runtime_error(aar_last_error());
    rr.det_err.resize(N);
    rr.keep.resize(N);
    rr.frame_stats.resize(4 * (size_t)data_->num_frames);
    return rr;
}

int64_t MultiCamMapper::reject_outliers(double k_median, double min_px, ResidualReport *out) {
    aar_outlier_rule rule;
    rule.struct_size = (uint32_t)sizeof rule;
    rule.k_median = k_median;
    rule.min_px = min_px;
    ResidualReport rr = residual_report(&rule);
    const int64_t dropped = rr.report.num_rejected;
    if (dropped > 0) {
        // data_->x_full (and with intrinsics cam_mats / dist_coeffs) is the current solution: the new data set starts from it
        aar_dataset *nd = nullptr;
        if (aar_dataset_select_observations(data_, rr.keep.data(), &nd)) throw std::runtime_error(aar_last_error());
        drop_problem();
        aar_dataset_free(data_);
        data_ = nd;
        mats2eVec();
    }
    if (out) *out = std::move(rr);
    return dropped;
}

bool MultiCamMapper::write_residuals_file(const std::string &path, const ResidualReport &rep) {
    if (!data_ || rep.keep.size() != (size_t)data_->num_obs) return false;   // (the list names the detections of the data set the report was made of)
    return aar_residual_report_write_yaml(path.c_str(), data_, rep.cam_stats.data(), rep.marker_stats.data(), rep.det_err.data(), rep.keep.data(),
                                          &rep.report) == AAR_OK;
}

MultiCamMapper::CornerPrediction MultiCamMapper::predict_corners(const std::vector<int> &cam_ids, const std::vector<int> &marker_ids,
                                                                 const std::vector<int> &frame_ids, bool covariance) {
    if (!data_) throw std::runtime_error("MultiCamMapper::predict_corners: no data set");
    if (cam_ids.size() != marker_ids.size() || cam_ids.size() != frame_ids.size())
        throw std::invalid_argument("MultiCamMapper::predict_corners: the three id lists differ in length");
    auto index_of = [](const int32_t *ids, int n, int id, const char *what) -> int32_t {
        const int32_t *e = ids + n, *p = std::lower_bound(ids, e, id);   // (ids ascending, as constraint_indices reads them)
        if (p == e || *p != id) throw std::invalid_argument(std::string("MultiCamMapper: no ") + what + " with id " + std::to_string(id));
        return (int32_t)(p - ids);
    };
    const size_t Q = cam_ids.size();
    std::vector<int32_t> qc(Q), qm(Q), qf(Q);
    for (size_t i = 0; i < Q; i++) {
        qc[i] = index_of(data_->cam_ids, data_->num_cams, cam_ids[i], "camera");
        qm[i] = index_of(data_->marker_ids, data_->num_markers, marker_ids[i], "marker");
        qf[i] = index_of(data_->frame_ids, data_->num_frames, frame_ids[i], "frame");
    }
    if (ensure_problem()) throw std::runtime_error(aar_last_error());
    CornerPrediction out;
    out.uv.assign(8 * std::max<size_t>(Q, 1), NAN);
    if (covariance) out.cov.assign(64 * std::max<size_t>(Q, 1), NAN);
    out.status.assign(std::max<size_t>(Q, 1), 0);
    out.report.struct_size = (uint32_t)sizeof out.report;
    std::vector<double> x = problem_vector();
    if (aar_problem_predict_corners(problem_, x.data(), (int64_t)Q, qc.data(), qm.data(), qf.data(), out.uv.data(), covariance ? out.cov.data() : nullptr,
                                    out.status.data(), &out.report))
        throw std::runtime_error(aar_last_error());
    out.uv.resize(8 * Q);
    out.status.resize(Q);
    if (covariance) {
        out.cov.resize(64 * Q);
        for (double &v : out.cov) v *= out.report.sigma2;
    }
    return out;
}

MultiCamMapper::DetectionLeverage MultiCamMapper::detection_leverage(bool rows) {
    if (!data_) throw std::runtime_error("MultiCamMapper::detection_leverage: no data set");
    if (ensure_problem()) throw std::runtime_error(aar_last_error());
    const size_t N = (size_t)data_->num_obs;
    DetectionLeverage out;
    out.leverage.assign(std::max<size_t>(N, 1), NAN);
    if (rows) out.row_leverage.assign(8 * std::max<size_t>(N, 1), NAN);
    out.report.struct_size = (uint32_t)sizeof out.report;
    std::vector<double> x = problem_vector();
    if (aar_problem_detection_leverage(problem_, x.data(), out.leverage.data(), rows ? out.row_leverage.data() : nullptr, &out.report))
        throw std::runtime_error(aar_last_error());
    out.leverage.resize(N);
    if (rows) out.row_leverage.resize(8 * N);
    return out;
}

bool MultiCamMapper::write_leverage_file(const std::string &path, const DetectionLeverage &lev, double h_min, const std::vector<double> &det_err) {
    if (!data_ || lev.leverage.size() != (size_t)data_->num_obs || (!det_err.empty() && det_err.size() != lev.leverage.size())) return false;
    return aar_leverage_write_yaml(path.c_str(), data_, lev.leverage.data(), det_err.empty() ? nullptr : det_err.data(), h_min, &lev.report) == AAR_OK;
}

MultiCamMapper::DetectionLoo MultiCamMapper::detection_loo(double f_max) {
    if (!data_) throw std::runtime_error("MultiCamMapper::detection_loo: no data set");
    if (ensure_problem()) throw std::runtime_error(aar_last_error());
    const size_t N = (size_t)data_->num_obs, n1 = std::max<size_t>(N, 1);
    DetectionLoo out;
    out.loo_resid.assign(8 * n1, NAN);
    for (std::vector<double> *v : {&out.q, &out.F, &out.cook, &out.leverage, &out.margin}) v->assign(n1, NAN);
    out.status.assign(n1, 0);
    out.keep.assign(n1, 1);
    out.report.struct_size = (uint32_t)sizeof out.report;
    aar_loo_rule rule;
    rule.struct_size = (uint32_t)sizeof rule;
    rule.f_max = f_max;
    std::vector<double> x = problem_vector();
    if (aar_problem_detection_loo(problem_, x.data(), f_max > 0.0 ? &rule : nullptr, out.loo_resid.data(), out.q.data(), out.F.data(), out.cook.data(),
                                  out.leverage.data(), out.margin.data(), out.status.data(), out.keep.data(), &out.report))
        throw std::runtime_error(aar_last_error());
    out.loo_resid.resize(8 * N);
    for (std::vector<double> *v : {&out.q, &out.F, &out.cook, &out.leverage, &out.margin}) v->resize(N);
    out.status.resize(N);
    out.keep.resize(N);
    return out;
}

MultiCamMapper::GateResult MultiCamMapper::gate_detections(const std::vector<int> &cam_ids, const std::vector<int> &marker_ids,
                                                           const std::vector<int> &frame_ids, const std::vector<float> &uv) {
    if (!data_) throw std::runtime_error("MultiCamMapper::gate_detections: no data set");
    const size_t Q = cam_ids.size();
    if (Q != marker_ids.size() || Q != frame_ids.size() || uv.size() != 8 * Q)
        throw std::invalid_argument("MultiCamMapper::gate_detections: the three id lists and uv / 8 differ in length");
    auto index_of = [](const int32_t *ids, int n, int id, const char *what) -> int32_t {
        const int32_t *e = ids + n, *p = std::lower_bound(ids, e, id);
        if (p == e || *p != id) throw std::invalid_argument(std::string("MultiCamMapper: no ") + what + " with id " + std::to_string(id));
        return (int32_t)(p - ids);
    };
    std::vector<int32_t> qc(Q), qm(Q), qf(Q);
    for (size_t i = 0; i < Q; i++) {
        qc[i] = index_of(data_->cam_ids, data_->num_cams, cam_ids[i], "camera");
        qm[i] = index_of(data_->marker_ids, data_->num_markers, marker_ids[i], "marker");
        qf[i] = index_of(data_->frame_ids, data_->num_frames, frame_ids[i], "frame");
    }
    if (ensure_problem()) throw std::runtime_error(aar_last_error());
    GateResult out;
    out.innovation.assign(8 * std::max<size_t>(Q, 1), NAN);
    out.chi2.assign(std::max<size_t>(Q, 1), NAN);
    out.status.assign(std::max<size_t>(Q, 1), 0);
    out.report.struct_size = (uint32_t)sizeof out.report;
    std::vector<double> x = problem_vector();
    if (aar_problem_gate_detections(problem_, x.data(), (int64_t)Q, qc.data(), qm.data(), qf.data(), Q ? uv.data() : nullptr, out.innovation.data(),
                                    out.chi2.data(), out.status.data(), &out.report))
        throw std::runtime_error(aar_last_error());
    out.innovation.resize(8 * Q);
    out.chi2.resize(Q);
    out.status.resize(Q);
    for (double &v : out.chi2) v /= out.report.sigma2;
    return out;
}

int64_t MultiCamMapper::reject_loo(double f_max, DetectionLoo *out) {
    DetectionLoo loo = detection_loo(f_max);
    // of every frame only the detection with the largest F among those the rule rejects goes (the first of them on a tie)
    std::vector<int64_t> worst((size_t)std::max(data_->num_frames, 1), -1);
    for (size_t o = 0; o < loo.keep.size(); o++) {
        if (loo.keep[o]) continue;
        int64_t &w = worst[data_->obs_frame[o]];
        if (w < 0 || loo.F[o] > loo.F[w]) w = (int64_t)o;
    }
    std::fill(loo.keep.begin(), loo.keep.end(), (uint8_t)1);
    int64_t dropped = 0;
    for (int64_t w : worst)
        if (w >= 0) { loo.keep[w] = 0; dropped++; }
    loo.report.rejected = dropped;
    if (dropped > 0) {
        aar_dataset *nd = nullptr;
        if (aar_dataset_select_observations(data_, loo.keep.data(), &nd)) throw std::runtime_error(aar_last_error());
        drop_problem();
        aar_dataset_free(data_);
        data_ = nd;
        mats2eVec();
    }
    if (out) *out = std::move(loo);
    return dropped;
}

bool MultiCamMapper::write_loo_file(const std::string &path, const DetectionLoo &loo, const std::vector<double> &det_err) {
    if (!data_ || loo.F.size() != (size_t)data_->num_obs || (!det_err.empty() && det_err.size() != loo.F.size())) return false;
    return aar_loo_write_yaml(path.c_str(), data_, loo.F.data(), loo.q.data(), loo.leverage.data(), det_err.empty() ? nullptr : det_err.data(),
                              loo.status.data(), loo.keep.data(), &loo.report) == AAR_OK;
}

void MultiCamMapper::error_function(const eVector &input, eVector &error) {
    if (probed(detail::EVAL_ERROR_FUNCTION)) return;
    if (!data_) throw std::runtime_error("MultiCamMapper::error_function: no data set");
    if (input.size() != get_num_vars(config_)) throw std::runtime_error("MultiCamMapper::error_function: input has not the Config's number of variables");
    if (ensure_problem()) throw std::runtime_error(aar_last_error());
    if (with_huber_ && aar_problem_set_huber_delta(problem_, hubberDelta)) throw std::runtime_error(aar_last_error());
    std::vector<double> x = problem_vector();
    if (aar_problem_merge_z(problem_, input.data(), x.data())) throw std::runtime_error(aar_last_error());
    error.assign(8 * (size_t)data_->num_obs, 0.0);
    if (aar_eval_residuals(problem_, x.data(), error.data(), nullptr)) throw std::runtime_error(aar_last_error());
}

void MultiCamMapper::jacobian_function(const eVector &, SparseJacobian<double> &) {
    if (probed(detail::EVAL_JACOBIAN_FUNCTION)) return;
    throw std::logic_error("MultiCamMapper::jacobian_function: the Jacobian is analytic and lives on the device (k_passA / k_passB accumulate its blocks "
                           "into J^T J); hand this function to SparseLevMarq::solve / step instead of calling it");
}

void MultiCamMapper::error_function_tracking(const eVector &, eVector &) {
    if (probed(detail::EVAL_ERROR_FUNCTION_TRACKING)) return;
    throw std::logic_error("MultiCamMapper::error_function_tracking: the per-frame residuals of tracking are evaluated inside k_track; hand this "
                           "function to SparseLevMarq::solve(z, f) (or call track()) instead of calling it");
}

// optCallBack, libs/multicam_mapper.cpp:412-417: the Huber delta schedule, driven by the solver's step callback
void MultiCamMapper::optCallBack(const eVector &) {
    if (hubberDelta > 2.5) hubberDelta -= 7.5 / 500;
    if (with_huber_ && problem_ && aar_problem_set_huber_delta(problem_, hubberDelta)) throw std::runtime_error(aar_last_error());
}

void MultiCamMapper::solve() {   // libs/multicam_mapper.cpp:419-428, statement for statement
    if (!data_) throw std::runtime_error("MultiCamMapper::solve: no data set");
    using namespace std::placeholders;
    mats2eVec();
    solver.setParams(solver_params);   // (the reference installs them in init(), :326-330; a mirror's caller may edit solver_params until here)
    solver.setStepCallBackFunc(std::bind(&MultiCamMapper::optCallBack, this, _1), /*needs_z=*/false);
    {   // error_function(io_vec, error); cout << error.dot(error): the sum alone, without bringing 8N residuals to the host
        std::vector<double> x_start;
        aar_problem *pb = detail::bind_problem(this, x_start);
        double e0 = 0;
        if (aar_eval_residuals(pb, x_start.data(), nullptr, &e0)) throw std::runtime_error(aar_last_error());
        std::cout << "initial_error: " << e0 << "error size: " << 8 * data_->num_obs << std::endl;  // :424
    }
    hubberDelta = 10;
    solver.solve(io_vec, std::bind(&MultiCamMapper::error_function, this, _1, _2), std::bind(&MultiCamMapper::jacobian_function, this, _1, _2));
    last_report = solver.report;
    eVec2Mats(io_vec);
}

// track(), libs/multicam_mapper.cpp:430-443.  The reference refines ONE frame per call (apps/track.cpp:127-131 re-inits the
// mapper with the frame's detections each time); here every frame held by the data set is refined in one launch, each with
// its own LM (detail::solve_tracking -> aar_track).
void MultiCamMapper::track() {
    if (!data_) throw std::runtime_error("MultiCamMapper::track: no data set");
    using namespace std::placeholders;
    mats2eVec();
    hubberDelta = 10;  // :439
    solver.setParams(solver_params);
    solver.solve(io_vec, std::bind(&MultiCamMapper::error_function_tracking, this, _1, _2));
    eVec2Mats(io_vec);
}

namespace detail {
double solve_tracking(MultiCamMapper *m, std::vector<double> &z) {
    std::vector<double> x;
    aar_problem *pb = bind_problem(m, x);
    if (z.size() != m->get_num_vars(m->config_)) throw std::runtime_error("SparseLevMarq::solve: z has not the Config's number of variables");
    if (aar_problem_merge_z(pb, z.data(), x.data())) throw std::runtime_error(aar_last_error());
    aar_lm_params p;
    aar_lm_default_params(&p);
    const SparseLevMarq<double>::Params &sp = m->solver._params;
    p.max_iters = sp.maxIters;
    p.min_error = sp.minError;
    p.min_step_error_diff = sp.min_step_error_diff;
    p.min_average_step_error_diff = sp.min_average_step_error_diff;
    p.tau = sp.tau;
    m->track_iterations.assign(m->data_->num_frames, 0);
    m->track_errors.assign(m->data_->num_frames, 0.0);
    if (aar_track(pb, x.data(), &p, m->track_iterations.data(), m->track_errors.data())) throw std::runtime_error(aar_last_error());
    if (aar_problem_extract_z(pb, x.data(), z.data())) throw std::runtime_error(aar_last_error());   // (only the frame poses have moved)
    memcpy(m->data_->x_full, x.data(), sizeof(double) * aar_dataset_full_len(m->data_));   // ... also when the Config keeps them out of z
    double e = 0;
    for (double v : m->track_errors) e += v;
    return e;
}
}  // namespace detail

// Smoothed tracking (aar_track_smooth): track()'s model plus a random-walk motion prior between consecutive frames, one
// joint LM on the device.  The mapper's frame ids are the prior's time axis, so a hole in the recording is bridged more loosely than one step.
void MultiCamMapper::track_smooth(double sigma_rot, double sigma_trans) {
    track_smooth(sigma_rot, sigma_trans, AAR_SMOOTH_MODEL_RANDOM_WALK, 0.0, 0.0);
}

// ... under either motion model: model = AAR_SMOOTH_MODEL_CONSTANT_VELOCITY makes sigma_rot / sigma_trans the deviation from
// constant velocity and sigma_rot0 / sigma_trans0 the prior on the first pair's motion
void MultiCamMapper::track_smooth(double sigma_rot, double sigma_trans, int model, double sigma_rot0, double sigma_trans0) {
    if (!data_) throw std::runtime_error("MultiCamMapper::track_smooth: no data set");
    mats2eVec();
    hubberDelta = 10;  // as track()
    std::vector<double> x;
    aar_problem *pb = detail::bind_problem(this, x);
    if (aar_problem_merge_z(pb, io_vec.data(), x.data())) throw std::runtime_error(aar_last_error());
    aar_lm_params p;
    aar_lm_default_params(&p);
    p.max_iters = solver_params.maxIters;
    p.min_error = solver_params.minError;
    p.min_step_error_diff = solver_params.min_step_error_diff;
    p.min_average_step_error_diff = solver_params.min_average_step_error_diff;
    p.tau = solver_params.tau;
    const int F = data_->num_frames;
    std::vector<double> time(F);
    for (int f = 0; f < F; f++) time[f] = (double)data_->frame_ids[f];
    aar_smooth_params sp;
    memset(&sp, 0, sizeof sp);
    sp.struct_size = sizeof sp;
    sp.sigma_rot = sigma_rot;
    sp.sigma_trans = sigma_trans;
    sp.frame_time = F ? time.data() : nullptr;
    sp.model = model;
    sp.sigma_rot0 = sigma_rot0;
    sp.sigma_trans0 = sigma_trans0;
    memset(&smooth_report, 0, sizeof smooth_report);
    smooth_report.struct_size = sizeof smooth_report;
    track_errors.assign(F, 0.0);
    smooth_pair_errors.assign(F > 1 ? F - 1 : 0, 0.0);
    if (aar_track_smooth(pb, x.data(), &p, &sp, track_errors.data(), smooth_pair_errors.data(), &smooth_report)) throw std::runtime_error(aar_last_error());
    if (aar_problem_extract_z(pb, x.data(), io_vec.data())) throw std::runtime_error(aar_last_error());   // (only the frame poses have moved)
    memcpy(data_->x_full, x.data(), sizeof(double) * aar_dataset_full_len(data_));   // ... also when the Config keeps them out of z
    eVec2Mats(io_vec);
}

// The pose covariance of the smoothed track (aar_track_smooth_covariance) at the current poses, under track_smooth()'s model
void MultiCamMapper::track_smooth_covariance(double sigma_rot, double sigma_trans, SmoothCovariance &out) {
    if (!data_) throw std::runtime_error("MultiCamMapper::track_smooth_covariance: no data set");
    mats2eVec();
    hubberDelta = 10;  // as track_smooth()
    std::vector<double> x;
    aar_problem *pb = detail::bind_problem(this, x);
    if (aar_problem_merge_z(pb, io_vec.data(), x.data())) throw std::runtime_error(aar_last_error());
    const int F = data_->num_frames;
    std::vector<double> time(F);
    for (int f = 0; f < F; f++) time[f] = (double)data_->frame_ids[f];
    aar_smooth_params sp;
    memset(&sp, 0, sizeof sp);
    sp.struct_size = sizeof sp;
    sp.sigma_rot = sigma_rot;
    sp.sigma_trans = sigma_trans;
    sp.frame_time = F ? time.data() : nullptr;
    out.frame_cov.assign(36 * (size_t)F, 0.0);
    out.lag_cov.assign(F > 1 ? 36 * (size_t)(F - 1) : 0, 0.0);
    out.lag2_cov.clear();
    memset(&out.report, 0, sizeof out.report);
    out.report.struct_size = sizeof out.report;
    if (aar_track_smooth_covariance(pb, x.data(), &sp, out.frame_cov.data(), out.lag_cov.data(), &out.report)) throw std::runtime_error(aar_last_error());
}

// ... under either motion model (aar_track_smooth_covariance2).  Constant velocity fills lag2_cov as well; the random walk
// leaves it empty (its selected inverse does not contain that block)
void MultiCamMapper::track_smooth_covariance(double sigma_rot, double sigma_trans, int model, double sigma_rot0, double sigma_trans0, SmoothCovariance &out) {
    if (!data_) throw std::runtime_error("MultiCamMapper::track_smooth_covariance: no data set");
    mats2eVec();
    hubberDelta = 10;  // as track_smooth()
    std::vector<double> x;
    aar_problem *pb = detail::bind_problem(this, x);
    if (aar_problem_merge_z(pb, io_vec.data(), x.data())) throw std::runtime_error(aar_last_error());
    const int F = data_->num_frames;
    std::vector<double> time(F);
    for (int f = 0; f < F; f++) time[f] = (double)data_->frame_ids[f];
    aar_smooth_params sp;
    memset(&sp, 0, sizeof sp);
    sp.struct_size = sizeof sp;
    sp.sigma_rot = sigma_rot;
    sp.sigma_trans = sigma_trans;
    sp.frame_time = F ? time.data() : nullptr;
    sp.model = model;
    sp.sigma_rot0 = sigma_rot0;
    sp.sigma_trans0 = sigma_trans0;
    const bool cv = model == AAR_SMOOTH_MODEL_CONSTANT_VELOCITY;
    out.frame_cov.assign(36 * (size_t)F, 0.0);
    out.lag_cov.assign(F > 1 ? 36 * (size_t)(F - 1) : 0, 0.0);
    out.lag2_cov.assign(cv && F > 2 ? 36 * (size_t)(F - 2) : 0, 0.0);
    memset(&out.report, 0, sizeof out.report);
    out.report.struct_size = sizeof out.report;
    // (an empty vector's data() may be anything: NULL says "not wanted", and under the random walk it must)
    if (aar_track_smooth_covariance2(pb, x.data(), &sp, out.frame_cov.data(), out.lag_cov.empty() ? nullptr : out.lag_cov.data(),
                                     out.lag2_cov.empty() ? nullptr : out.lag2_cov.data(), &out.report))
        throw std::runtime_error(aar_last_error());
}

// The smoothed track at any time (aar_track_smooth_query) from the current poses, under track_smooth()'s model
void MultiCamMapper::track_smooth_query(double sigma_rot, double sigma_trans, const std::vector<double> &query_time, SmoothQuery &out, bool covariance) {
    if (!data_) throw std::runtime_error("MultiCamMapper::track_smooth_query: no data set");
    mats2eVec();
    hubberDelta = 10;  // as track_smooth()
    std::vector<double> x;
    aar_problem *pb = detail::bind_problem(this, x);
    if (aar_problem_merge_z(pb, io_vec.data(), x.data())) throw std::runtime_error(aar_last_error());
    const int F = data_->num_frames;
    std::vector<double> time(F);
    for (int f = 0; f < F; f++) time[f] = (double)data_->frame_ids[f];
    aar_smooth_params sp;
    memset(&sp, 0, sizeof sp);
    sp.struct_size = sizeof sp;
    sp.sigma_rot = sigma_rot;
    sp.sigma_trans = sigma_trans;
    sp.frame_time = F ? time.data() : nullptr;
    const size_t n = query_time.size();
    out.pose.assign(6 * n, 0.0);
    out.cov.assign(covariance ? 36 * n : 0, 0.0);
    out.segment.assign(n, 0);
    memset(&out.report, 0, sizeof out.report);
    out.report.struct_size = sizeof out.report;
    if (aar_track_smooth_query(pb, x.data(), &sp, (int64_t)n, query_time.data(), out.pose.data(), covariance ? out.cov.data() : nullptr,
                               out.segment.data(), &out.report))
        throw std::runtime_error(aar_last_error());
}

// ... under the motion model AAR_SMOOTH_MODEL_* (aar_track_smooth_query2).  Constant velocity: one Gauss-Newton step of the
// smoother for a frame without detections inserted at each time; the random walk is the call above
void MultiCamMapper::track_smooth_query(double sigma_rot, double sigma_trans, int model, double sigma_rot0, double sigma_trans0,
                                        const std::vector<double> &query_time, SmoothQuery &out, bool covariance) {
    if (!data_) throw std::runtime_error("MultiCamMapper::track_smooth_query: no data set");
    mats2eVec();
    hubberDelta = 10;  // as track_smooth()
    std::vector<double> x;
    aar_problem *pb = detail::bind_problem(this, x);
    if (aar_problem_merge_z(pb, io_vec.data(), x.data())) throw std::runtime_error(aar_last_error());
    const int F = data_->num_frames;
    std::vector<double> time(F);
    for (int f = 0; f < F; f++) time[f] = (double)data_->frame_ids[f];
    aar_smooth_params sp;
    memset(&sp, 0, sizeof sp);
    sp.struct_size = sizeof sp;
    sp.sigma_rot = sigma_rot;
    sp.sigma_trans = sigma_trans;
    sp.frame_time = F ? time.data() : nullptr;
    sp.model = model;
    sp.sigma_rot0 = sigma_rot0;
    sp.sigma_trans0 = sigma_trans0;
    const size_t n = query_time.size();
    out.pose.assign(6 * n, 0.0);
    out.cov.assign(covariance ? 36 * n : 0, 0.0);
    out.segment.assign(n, 0);
    memset(&out.report, 0, sizeof out.report);
    out.report.struct_size = sizeof out.report;
    if (aar_track_smooth_query2(pb, x.data(), &sp, (int64_t)n, query_time.data(), out.pose.data(), covariance ? out.cov.data() : nullptr,
                                out.segment.data(), &out.report))
        throw std::runtime_error(aar_last_error());
}

// The covariance between any two frames and the relative motion between them (aar_track_smooth_relative) from the current
// poses, under track_smooth()'s prior
void MultiCamMapper::track_smooth_relative(double sigma_rot, double sigma_trans, int model, double sigma_rot0, double sigma_trans0,
                                           const std::vector<std::pair<int32_t, int32_t>> &pairs, SmoothRelative &out) {
    if (!data_) throw std::runtime_error("MultiCamMapper::track_smooth_relative: no data set");
    mats2eVec();
    hubberDelta = 10;  // as track_smooth()
    std::vector<double> x;
    aar_problem *pb = detail::bind_problem(this, x);
    if (aar_problem_merge_z(pb, io_vec.data(), x.data())) throw std::runtime_error(aar_last_error());
    const int F = data_->num_frames;
    std::vector<double> time(F);
    for (int f = 0; f < F; f++) time[f] = (double)data_->frame_ids[f];
    aar_smooth_params sp;
    memset(&sp, 0, sizeof sp);
    sp.struct_size = sizeof sp;
    sp.sigma_rot = sigma_rot;
    sp.sigma_trans = sigma_trans;
    sp.frame_time = F ? time.data() : nullptr;
    sp.model = model;
    sp.sigma_rot0 = sigma_rot0;
    sp.sigma_trans0 = sigma_trans0;
    const size_t n = pairs.size();
    std::vector<int32_t> fa(n), fb(n);
    for (size_t i = 0; i < n; i++) { fa[i] = pairs[i].first; fb[i] = pairs[i].second; }
    out.cross_cov.assign(36 * n, 0.0);
    out.rel.assign(6 * n, 0.0);
    out.rel_cov.assign(36 * n, 0.0);
    memset(&out.report, 0, sizeof out.report);
    out.report.struct_size = sizeof out.report;
    if (aar_track_smooth_relative(pb, x.data(), &sp, (int64_t)n, fa.data(), fb.data(), out.cross_cov.data(), out.rel.data(), out.rel_cov.data(),
                                  &out.report))
        throw std::runtime_error(aar_last_error());
}

// The per-detection layer of the smoothed track from the current poses, under track_smooth()'s prior
namespace {
struct SmoothBound {   // what every entry of the layer starts from: the bound problem, its pose vector, the frame ids as times, the parameters
    aar_problem *pb = nullptr;
    std::vector<double> x, time;
    aar_smooth_params sp;
};
int32_t index_of_id(const int32_t *ids, int n, int id, const char *what) {
    const int32_t *e = ids + n, *p = std::lower_bound(ids, e, id);
    if (p == e || *p != id) throw std::invalid_argument(std::string("MultiCamMapper: no ") + what + " with id " + std::to_string(id));
    return (int32_t)(p - ids);
}
}  // namespace

#define AAR_SMOOTH_BOUND(b, who)                                                                                        \
    if (!data_) throw std::runtime_error("MultiCamMapper::" who ": no data set");                                       \
    mats2eVec();                                                                                                        \
    hubberDelta = 10; /* as track_smooth() */                                                                           \
    SmoothBound b;                                                                                                      \
    b.pb = detail::bind_problem(this, b.x);                                                                             \
    if (aar_problem_merge_z(b.pb, io_vec.data(), b.x.data())) throw std::runtime_error(aar_last_error());               \
    b.time.resize(data_->num_frames);                                                                                   \
    for (int f = 0; f < data_->num_frames; f++) b.time[f] = (double)data_->frame_ids[f];                                \
    memset(&b.sp, 0, sizeof b.sp);                                                                                      \
    b.sp.struct_size = sizeof b.sp;                                                                                     \
    b.sp.sigma_rot = sigma_rot;                                                                                         \
    b.sp.sigma_trans = sigma_trans;                                                                                     \
    b.sp.frame_time = data_->num_frames ? b.time.data() : nullptr;                                                      \
    b.sp.model = model;                                                                                                 \
    b.sp.sigma_rot0 = sigma_rot0;                                                                                       \
    b.sp.sigma_trans0 = sigma_trans0

void MultiCamMapper::track_smooth_detection_leverage(double sigma_rot, double sigma_trans, int model, double sigma_rot0, double sigma_trans0,
                                                     SmoothLeverage &out) {
    AAR_SMOOTH_BOUND(b, "track_smooth_detection_leverage");
    const size_t N = (size_t)data_->num_obs, n1 = std::max<size_t>(N, 1);
    out.leverage.assign(n1, NAN);
    out.row_leverage.assign(8 * n1, NAN);
    memset(&out.report, 0, sizeof out.report);
    out.report.struct_size = sizeof out.report;
    if (aar_track_smooth_detection_leverage(b.pb, b.x.data(), &b.sp, out.leverage.data(), out.row_leverage.data(), &out.report))
        throw std::runtime_error(aar_last_error());
    out.leverage.resize(N);
    out.row_leverage.resize(8 * N);
}

void MultiCamMapper::track_smooth_detection_loo(double sigma_rot, double sigma_trans, int model, double sigma_rot0, double sigma_trans0, double f_max,
                                                SmoothLoo &out) {
    AAR_SMOOTH_BOUND(b, "track_smooth_detection_loo");
    const size_t N = (size_t)data_->num_obs, n1 = std::max<size_t>(N, 1);
    out.loo_resid.assign(8 * n1, NAN);
    for (std::vector<double> *v : {&out.q, &out.F, &out.cook, &out.leverage, &out.margin}) v->assign(n1, NAN);
    out.status.assign(n1, 0);
    out.keep.assign(n1, 1);
    memset(&out.report, 0, sizeof out.report);
    out.report.struct_size = sizeof out.report;
    aar_loo_rule rule;
    rule.struct_size = (uint32_t)sizeof rule;
    rule.f_max = f_max;
    if (aar_track_smooth_detection_loo(b.pb, b.x.data(), &b.sp, f_max > 0.0 ? &rule : nullptr, out.loo_resid.data(), out.q.data(), out.F.data(),
                                       out.cook.data(), out.leverage.data(), out.margin.data(), out.status.data(), out.keep.data(), &out.report))
        throw std::runtime_error(aar_last_error());
    out.loo_resid.resize(8 * N);
    for (std::vector<double> *v : {&out.q, &out.F, &out.cook, &out.leverage, &out.margin}) v->resize(N);
    out.status.resize(N);
    out.keep.resize(N);
}

void MultiCamMapper::track_smooth_predict_corners(double sigma_rot, double sigma_trans, int model, double sigma_rot0, double sigma_trans0,
                                                  const std::vector<int> &cam_ids, const std::vector<int> &marker_ids,
                                                  const std::vector<double> &times, SmoothCorners &out, bool covariance) {
    const size_t Q = cam_ids.size(), q1 = std::max<size_t>(Q, 1);
    if (Q != marker_ids.size() || Q != times.size())
        throw std::invalid_argument("MultiCamMapper::track_smooth_predict_corners: the id lists and the times differ in length");
    AAR_SMOOTH_BOUND(b, "track_smooth_predict_corners");
    std::vector<int32_t> qc(Q), qm(Q);
    for (size_t i = 0; i < Q; i++) {
        qc[i] = index_of_id(data_->cam_ids, data_->num_cams, cam_ids[i], "camera");
        qm[i] = index_of_id(data_->marker_ids, data_->num_markers, marker_ids[i], "marker");
    }
    out.uv.assign(8 * q1, NAN);
    out.cov.assign(covariance ? 64 * q1 : 0, NAN);
    out.m2.clear();
    out.status.assign(q1, 0);
    out.segment.assign(q1, 0);
    memset(&out.report, 0, sizeof out.report);
    out.report.struct_size = sizeof out.report;
    if (aar_track_smooth_predict_corners(b.pb, b.x.data(), &b.sp, (int64_t)Q, qc.data(), qm.data(), times.data(), out.uv.data(),
                                         covariance ? out.cov.data() : nullptr, out.status.data(), out.segment.data(), &out.report))
        throw std::runtime_error(aar_last_error());
    out.uv.resize(8 * Q);
    if (covariance) out.cov.resize(64 * Q);
    out.status.resize(Q);
    out.segment.resize(Q);
}

void MultiCamMapper::track_smooth_gate_detections(double sigma_rot, double sigma_trans, int model, double sigma_rot0, double sigma_trans0,
                                                  const std::vector<int> &cam_ids, const std::vector<int> &marker_ids,
                                                  const std::vector<double> &times, const std::vector<float> &uv_obs, SmoothCorners &out) {
    const size_t Q = cam_ids.size(), q1 = std::max<size_t>(Q, 1);
    if (Q != marker_ids.size() || Q != times.size() || uv_obs.size() != 8 * Q)
        throw std::invalid_argument("MultiCamMapper::track_smooth_gate_detections: the id lists, the times and uv / 8 differ in length");
    AAR_SMOOTH_BOUND(b, "track_smooth_gate_detections");
    std::vector<int32_t> qc(Q), qm(Q);
    for (size_t i = 0; i < Q; i++) {
        qc[i] = index_of_id(data_->cam_ids, data_->num_cams, cam_ids[i], "camera");
        qm[i] = index_of_id(data_->marker_ids, data_->num_markers, marker_ids[i], "marker");
    }
    out.uv.assign(8 * q1, NAN);
    out.cov.clear();
    out.m2.assign(q1, NAN);
    out.status.assign(q1, 0);
    out.segment.assign(q1, 0);
    memset(&out.report, 0, sizeof out.report);
    out.report.struct_size = sizeof out.report;
    if (aar_track_smooth_gate_detections(b.pb, b.x.data(), &b.sp, (int64_t)Q, qc.data(), qm.data(), times.data(), Q ? uv_obs.data() : nullptr,
                                         out.uv.data(), out.m2.data(), out.status.data(), out.segment.data(), &out.report))
        throw std::runtime_error(aar_last_error());
    out.uv.resize(8 * Q);
    out.m2.resize(Q);
    out.status.resize(Q);
    out.segment.resize(Q);
}

int64_t MultiCamMapper::smooth_reject_loo(double sigma_rot, double sigma_trans, int model, double sigma_rot0, double sigma_trans0, double f_max,
                                          SmoothLoo *out) {
    SmoothLoo loo;
    track_smooth_detection_loo(sigma_rot, sigma_trans, model, sigma_rot0, sigma_trans0, f_max, loo);
    // of every frame only the detection with the largest F among those the rule rejects goes (the first of them on a tie), as reject_loo
    std::vector<int64_t> worst((size_t)std::max(data_->num_frames, 1), -1);
    for (size_t o = 0; o < loo.keep.size(); o++) {
        if (loo.keep[o]) continue;
        int64_t &w = worst[data_->obs_frame[o]];
        if (w < 0 || loo.F[o] > loo.F[w]) w = (int64_t)o;
    }
    std::fill(loo.keep.begin(), loo.keep.end(), (uint8_t)1);
    int64_t dropped = 0;
    for (int64_t w : worst)
        if (w >= 0) { loo.keep[w] = 0; dropped++; }
    loo.report.rejected = dropped;
    if (dropped > 0) {
        aar_dataset *nd = nullptr;
        if (aar_dataset_select_observations(data_, loo.keep.data(), &nd)) throw std::runtime_error(aar_last_error());
        drop_problem();
        aar_dataset_free(data_);
        data_ = nd;
        mats2eVec();
    }
    if (out) *out = std::move(loo);
    return dropped;
}
#undef AAR_SMOOTH_BOUND

// The pixel noise and the motion sigmas fitted to the sequence itself (aar_track_smooth_fit), under track_smooth()'s model
// (the frame ids as the time axis).  The frame poses end as the smoothed track at the fitted values.
void MultiCamMapper::fit_smooth_sigmas(double sigma_rot, double sigma_trans, SmoothFit &out, const aar_smooth_fit_params *fit) {
    fit_smooth_sigmas(sigma_rot, sigma_trans, AAR_SMOOTH_MODEL_RANDOM_WALK, 0.0, 0.0, out, fit);
}

// ... under the motion model AAR_SMOOTH_MODEL_* (aar_track_smooth_fit2).  Constant velocity: sigma_rot / sigma_trans are the
// start values of the second-difference terms, sigma_rot0 / sigma_trans0 the first pair's PHYSICAL sigmas, held; the random walk is the call above
void MultiCamMapper::fit_smooth_sigmas(double sigma_rot, double sigma_trans, int model, double sigma_rot0, double sigma_trans0, SmoothFit &out,
                                       const aar_smooth_fit_params *fit) {
    if (!data_) throw std::runtime_error("MultiCamMapper::fit_smooth_sigmas: no data set");
    mats2eVec();
    hubberDelta = 10;  // as track_smooth() (a mapper set_with_huber(true) is refused by the library: the fit needs the Gaussian data model)
    std::vector<double> x;
    aar_problem *pb = detail::bind_problem(this, x);
    if (aar_problem_merge_z(pb, io_vec.data(), x.data())) throw std::runtime_error(aar_last_error());
    aar_lm_params p;
    aar_lm_default_params(&p);
    p.max_iters = solver_params.maxIters;
    p.min_error = solver_params.minError;
    p.min_step_error_diff = solver_params.min_step_error_diff;
    p.min_average_step_error_diff = solver_params.min_average_step_error_diff;
    p.tau = solver_params.tau;
    const int F = data_->num_frames;
    std::vector<double> time(F);
    for (int f = 0; f < F; f++) time[f] = (double)data_->frame_ids[f];
    aar_smooth_params sp;
    memset(&sp, 0, sizeof sp);
    sp.struct_size = sizeof sp;
    sp.sigma_rot = sigma_rot;
    sp.sigma_trans = sigma_trans;
    sp.frame_time = F ? time.data() : nullptr;
    sp.model = model;
    sp.sigma_rot0 = sigma_rot0;
    sp.sigma_trans0 = sigma_trans0;
    aar_smooth_fit_params fp;
    aar_smooth_fit_default_params(&fp);
    if (fit) {
        if (aar_smooth_fit_params_validate(fit)) throw std::runtime_error(aar_last_error());
        memcpy(&fp, fit, std::min<size_t>(fit->struct_size, sizeof fp));
        fp.struct_size = sizeof fp;
    }
    out.path.assign(3 * ((size_t)fp.max_iters + 1), 0.0);
    memset(&out.report, 0, sizeof out.report);
    out.report.struct_size = sizeof out.report;
    if (aar_track_smooth_fit2(pb, x.data(), &p, &sp, &fp, out.path.data(), &out.report)) throw std::runtime_error(aar_last_error());
    out.path.resize(3 * ((size_t)out.report.iterations + 1));
    if (aar_problem_extract_z(pb, x.data(), io_vec.data())) throw std::runtime_error(aar_last_error());   // (only the frame poses have moved)
    memcpy(data_->x_full, x.data(), sizeof(double) * aar_dataset_full_len(data_));   // ... also when the Config keeps them out of z
    eVec2Mats(io_vec);
}

// The live loop over the data set's frames (aar_tracker_*): what apps/track.cpp does per incoming frame, with the
// mapper's own frames as the stream.
namespace {
// the covariance blocks of the window after a push: a frame keeps those of the last push it was in the window of -- its lagged block
void take_live_covariance(LiveTracker &lt, MultiCamMapper::LiveCovariance *cov) {
    if (!cov) return;
    const aar_tracker_uncertainty_record u = lt.uncertainty();
    for (int i = 0; i < u.window_frames; i++) {
        const size_t f = (size_t)u.frame_index[i];
        memcpy(&cov->frame_cov[36 * f], u.cov[i], sizeof u.cov[i]);
        cov->sigma2[f] = u.sigma2;
        cov->valid[f] = u.cov_valid ? 1 : 0;
    }
}
// the gate on (gate != NULL), and room for every frame's record
void start_live_gate(LiveTracker &lt, const aar_tracker_gate_params *gate, int F, std::vector<aar_tracker_gate_info> &out) {
    out.clear();
    if (!gate) return;
    lt.enable_gate(gate);
    out.assign((size_t)F, aar_tracker_gate_info());
}
// the motion model on (motion != NULL), and room for every frame's record
void start_live_motion(LiveTracker &lt, const aar_tracker_motion_params *motion, int F, std::vector<aar_tracker_motion_info> &out) {
    out.clear();
    if (!motion) return;
    lt.enable_motion(motion);
    if (motion->model != AAR_TRACKER_MOTION_RANDOM_WALK) out.assign((size_t)F, aar_tracker_motion_info());
}
void size_live_covariance(MultiCamMapper::LiveCovariance *cov, int F) {
    if (!cov) return;
    cov->frame_cov.assign(36 * (size_t)F, 0.0);
    cov->sigma2.assign((size_t)F, 0.0);
    cov->valid.assign((size_t)F, 0);
}
}  // namespace

void MultiCamMapper::track_live(int lag, bool smooth, double sigma_rot, double sigma_trans, int anchor_mode, LiveCovariance *covariance,
                                const aar_tracker_gate_params *gate, const aar_tracker_motion_params *motion) {
    if (!data_) throw std::runtime_error("MultiCamMapper::track_live: no data set");
    hubberDelta = 10;  // as track()
    const int F = data_->num_frames;
    std::vector<int64_t> start(F + 1, 0);
    for (int64_t o = 0; o < data_->num_obs; o++) start[data_->obs_frame[o] + 1]++;
    int64_t most = 1;
    for (int f = 0; f < F; f++) { most = std::max(most, start[f + 1]); start[f + 1] += start[f]; }
    LiveTracker::Options o;
    o.lag = lag; o.smooth = smooth; o.sigma_rot = sigma_rot; o.sigma_trans = sigma_trans;
    o.with_huber = with_huber_; o.huber_delta = hubberDelta; o.max_obs_per_frame = (int)most; o.device_id = device_id;
    o.anchor_mode = anchor_mode; o.covariance = covariance != nullptr;
    LiveTracker lt(*this, o, &solver_params);
    size_live_covariance(covariance, F);
    start_live_gate(lt, gate, F, live_gates);
    start_live_motion(lt, motion, F, live_motions);
    PoseLayout L;
    L.C = data_->num_cams; L.M = data_->num_markers; L.F = F;
    std::vector<double> z(data_->x_full + L.full_fr0(), data_->x_full + L.full_fr0() + 6LL * F);
    live_results.assign(F, aar_tracker_result());
    std::vector<LiveTracker::Detection> det;
    for (int f = 0; f < F; f++) {
        det.clear();
        for (int64_t k = start[f]; k < start[f + 1]; k++) {
            LiveTracker::Detection d;
            d.cam_id = data_->cam_ids[data_->obs_cam[k]];
            d.marker_id = data_->marker_ids[data_->obs_marker[k]];
            memcpy(d.uv, data_->obs_uv + 8 * k, sizeof d.uv);
            det.push_back(d);
        }
        const aar_tracker_result r = lt.push((double)data_->frame_ids[f], det, data_->x_full + L.full_fr0() + 6LL * f);
        live_results[f] = r;
        if (gate) live_gates[f] = lt.last_gate();
        if (!live_motions.empty()) live_motions[f] = lt.last_motion();
        take_live_covariance(lt, covariance);
        if (r.has_lagged) memcpy(&z[6 * (size_t)r.lagged_index], r.lagged_pose, sizeof r.lagged_pose);
    }
    const LiveTracker::Window w = lt.window();   // the frames that never left the window
    for (size_t i = 0; i < w.frame_index.size(); i++) memcpy(&z[6 * (size_t)w.frame_index[i]], w.poses[i].data(), 6 * sizeof(double));
    memcpy(data_->x_full + L.full_fr0(), z.data(), z.size() * sizeof(double));
    mats2eVec();
}

void MultiCamMapper::track_live_from_detections(const aar_detections *det, const std::vector<aar_cam_model> &cams, int lag, bool smooth, double sigma_rot,
                                                double sigma_trans, int start_policy, int anchor_mode, LiveCovariance *covariance,
                                                const aar_tracker_gate_params *gate, const aar_tracker_motion_params *motion) {
    if (!data_ || !det) throw std::runtime_error("MultiCamMapper::track_live_from_detections: no data set / no detections");
    hubberDelta = 10;  // as track()
    const int F = data_->num_frames;
    // the detections of every frame id, in file order
    std::map<int, std::vector<int64_t>> of_frame;
    size_t most = 1;
    for (int64_t i = 0; i < det->num_det; i++) {
        std::vector<int64_t> &v = of_frame[det->det_frame[i]];
        v.push_back(i);
        most = std::max(most, v.size());
    }
    LiveTracker::Options o;
    o.lag = lag; o.smooth = smooth; o.sigma_rot = sigma_rot; o.sigma_trans = sigma_trans;
    o.with_huber = with_huber_; o.huber_delta = hubberDelta; o.max_obs_per_frame = (int)most; o.device_id = device_id;
    o.anchor_mode = anchor_mode; o.covariance = covariance != nullptr;
    LiveTracker lt(*this, o, &solver_params);
    size_live_covariance(covariance, F);
    LiveTracker::DetectionOptions dopt;
    for (int c = 0; c < data_->num_cams; c++) {
        const int id = data_->cam_ids[c];
        if (id < 0 || id >= (int)cams.size()) throw std::runtime_error("MultiCamMapper::track_live_from_detections: no calibration for camera " + std::to_string(id));
        dopt.cams[id] = cams[id];
    }
    dopt.start_policy = start_policy;
    lt.enable_detections(dopt);
    start_live_gate(lt, gate, F, live_gates);
    start_live_motion(lt, motion, F, live_motions);
    PoseLayout L;
    L.C = data_->num_cams; L.M = data_->num_markers; L.F = F;
    std::vector<double> z(data_->x_full + L.full_fr0(), data_->x_full + L.full_fr0() + 6LL * F);
    live_results.assign(F, aar_tracker_result());
    live_starts.assign(F, aar_tracker_start_info());
    std::vector<LiveTracker::Detection> dets;
    for (int f = 0; f < F; f++) {
        dets.clear();
        const auto it = of_frame.find(data_->frame_ids[f]);
        if (it != of_frame.end())
            for (int64_t k : it->second) {
                LiveTracker::Detection d;
                d.cam_id = det->det_cam[k];
                d.marker_id = det->det_id[k];
                memcpy(d.uv, det->det_uv + 8 * k, sizeof d.uv);
                dets.push_back(d);
            }
        const aar_tracker_result r = lt.push_detections((double)data_->frame_ids[f], dets, nullptr, &live_starts[f]);
        live_results[f] = r;
        if (gate) live_gates[f] = lt.last_gate();
        if (!live_motions.empty()) live_motions[f] = lt.last_motion();
        take_live_covariance(lt, covariance);
        if (r.has_lagged) memcpy(&z[6 * (size_t)r.lagged_index], r.lagged_pose, sizeof r.lagged_pose);
    }
    const LiveTracker::Window w = lt.window();   // the frames that never left the window
    for (size_t i = 0; i < w.frame_index.size(); i++) memcpy(&z[6 * (size_t)w.frame_index[i]], w.poses[i].data(), 6 * sizeof(double));
    memcpy(data_->x_full + L.full_fr0(), z.data(), z.size() * sizeof(double));
    mats2eVec();
}

bool MultiCamMapper::write_live_covariance_file(const std::string &path, const LiveCovariance &cov) {
    if (!data_ || cov.valid.size() != (size_t)data_->num_frames) return false;
    return aar_tracker_covariance_write_yaml(path.c_str(), data_, cov.frame_cov.data(), cov.sigma2.data(), cov.valid.data()) == AAR_OK;
}

// ---- what LiveTracker and LiveTrackerBank share ----
namespace {

aar_tracker_params live_params(const LiveTracker::Options &o) {
    aar_tracker_params p;
    aar_tracker_default_params(&p);
    p.lag = o.lag; p.smooth = o.smooth ? 1 : 0; p.sigma_rot = o.sigma_rot; p.sigma_trans = o.sigma_trans;
    p.with_huber = o.with_huber ? 1 : 0; p.huber_delta = o.huber_delta; p.max_obs_per_frame = o.max_obs_per_frame; p.device_id = o.device_id;
    p.anchor_mode = o.anchor_mode; p.covariance = o.covariance ? 1 : 0;
    return p;
}

aar_lm_params live_lm_params(const SparseLevMarq<double>::Params *lm) {
    aar_lm_params q;
    aar_lm_default_params(&q);
    if (lm) {
        q.max_iters = lm->maxIters; q.min_error = lm->minError; q.min_step_error_diff = lm->min_step_error_diff;
        q.min_average_step_error_diff = lm->min_average_step_error_diff; q.tau = lm->tau;
    }
    return q;
}

void live_index_ids(const aar_dataset *d, std::map<int, int> &cam_index, std::map<int, int> &marker_index) {
    for (int c = 0; c < d->num_cams; c++) cam_index[d->cam_ids[c]] = c;
    for (int m = 0; m < d->num_markers; m++) marker_index[d->marker_ids[m]] = m;
}

// appends the detections of known cameras and markers by INDEX; returns how many
int32_t live_append(const std::map<int, int> &cam_index, const std::map<int, int> &marker_index, const std::vector<LiveTracker::Detection> &detections,
                    std::vector<int32_t> &cam, std::vector<int32_t> &marker, std::vector<float> &uv) {
    int32_t n = 0;
    for (const LiveTracker::Detection &d : detections) {
        const auto c = cam_index.find(d.cam_id);
        const auto m = marker_index.find(d.marker_id);
        if (c == cam_index.end() || m == marker_index.end()) continue;
        cam.push_back(c->second);
        marker.push_back(m->second);
        uv.insert(uv.end(), d.uv, d.uv + 8);
        n++;
    }
    return n;
}

// o as aar_tracker_detection_params; by_index keeps the calibrations p.cams points to
aar_tracker_detection_params live_detection_params(const std::map<int, int> &cam_index, const LiveTracker::DetectionOptions &o,
                                                   std::vector<aar_cam_model> &by_index, const char *who) {
    aar_tracker_detection_params p;
    aar_tracker_default_detection_params(&p);
    if (!o.cams.empty()) {
        by_index.resize(cam_index.size());
        for (const auto &ci : cam_index) {
            const auto it = o.cams.find(ci.first);
            if (it == o.cams.end()) throw std::runtime_error(std::string(who) + "::enable_detections: no calibration for camera " + std::to_string(ci.first));
            by_index[ci.second] = it->second;
        }
        p.cams = by_index.data();
    }
    p.ippe_threshold = o.ippe_threshold; p.min_detections = o.min_detections; p.start_policy = o.start_policy;
    return p;
}

LiveTracker::Window live_window(int32_t n, const int64_t *idx, const double *poses, const double *fe, const double *pe, const double *anchor, int32_t has) {
    LiveTracker::Window w;
    for (int i = 0; i < n; i++) {
        w.frame_index.push_back(idx[i]);
        std::array<double, 6> z;
        memcpy(z.data(), poses + 6 * i, sizeof z);
        w.poses.push_back(z);
        w.frame_err.push_back(fe[i]);
        w.pair_err.push_back(pe[i]);
    }
    w.has_anchor = has != 0;
    if (has) memcpy(w.anchor_pose.data(), anchor, 6 * sizeof(double));
    return w;
}

aar_tracker_result blank_result() {
    aar_tracker_result r;
    memset(&r, 0, sizeof r);
    r.struct_size = sizeof r;
    return r;
}

}  // namespace

LiveTracker::LiveTracker(const MultiCamMapper &solution, const Options &o, const SparseLevMarq<double>::Params *lm) {
    const aar_dataset *d = solution.dataset();
    if (!d) throw std::runtime_error("LiveTracker: the mapper holds no solution");
    live_index_ids(d, cam_index_, marker_index_);
    const aar_tracker_params p = live_params(o);
    const aar_lm_params q = live_lm_params(lm);
    if (aar_tracker_create(d, &p, &q, &tracker_)) throw std::runtime_error(aar_last_error());
}

LiveTracker::~LiveTracker() { aar_tracker_destroy(tracker_); }

aar_tracker_result LiveTracker::push(double frame_time, const std::vector<Detection> &detections, const double *start) {
    cam_.clear(); marker_.clear(); uv_.clear();
    const int32_t n = live_append(cam_index_, marker_index_, detections, cam_, marker_, uv_);
    aar_tracker_result r = blank_result();
    if (aar_tracker_push(tracker_, frame_time, n, cam_.data(), marker_.data(), uv_.data(), start, &r)) throw std::runtime_error(aar_last_error());
    return r;
}

void LiveTracker::enable_detections(const DetectionOptions &o) {
    std::vector<aar_cam_model> by_index;
    const aar_tracker_detection_params p = live_detection_params(cam_index_, o, by_index, "LiveTracker");
    if (aar_tracker_enable_detections(tracker_, &p)) throw std::runtime_error(aar_last_error());
}

aar_tracker_result LiveTracker::push_detections(double frame_time, const std::vector<Detection> &detections, const double *start,
                                                aar_tracker_start_info *info) {
    cam_.clear(); marker_.clear(); uv_.clear();
    const int32_t n = live_append(cam_index_, marker_index_, detections, cam_, marker_, uv_);
    aar_tracker_result r = blank_result();
    if (info) { memset(info, 0, sizeof *info); info->struct_size = sizeof *info; }
    if (aar_tracker_push_detections(tracker_, frame_time, n, cam_.data(), marker_.data(), uv_.data(), start, &r, info))
        throw std::runtime_error(aar_last_error());
    return r;
}

void LiveTracker::enable_gate(const aar_tracker_gate_params *params) {
    aar_tracker_gate_params p;
    aar_tracker_default_gate_params(&p);
    if (aar_tracker_enable_gate(tracker_, params ? params : &p)) throw std::runtime_error(aar_last_error());
}

void LiveTracker::enable_motion(const aar_tracker_motion_params *params) {
    aar_tracker_motion_params p;
    aar_tracker_default_motion_params(&p);
    if (aar_tracker_enable_motion(tracker_, params ? params : &p)) throw std::runtime_error(aar_last_error());
}

aar_tracker_motion_info LiveTracker::last_motion() {
    aar_tracker_motion_info m;
    memset(&m, 0, sizeof m);
    m.struct_size = (uint32_t)sizeof m;
    if (aar_tracker_last_motion(tracker_, &m)) throw std::runtime_error(aar_last_error());
    return m;
}

std::array<double, 6> LiveTracker::predict(double time) {
    std::array<double, 6> pose;
    if (aar_tracker_predict(tracker_, time, pose.data())) throw std::runtime_error(aar_last_error());
    return pose;
}

aar_tracker_gate_info LiveTracker::last_gate() {
    aar_tracker_gate_info g;
    memset(&g, 0, sizeof g);
    g.struct_size = sizeof g;
    if (aar_tracker_last_gate(tracker_, &g)) throw std::runtime_error(aar_last_error());
    return g;
}

void LiveTracker::gate_detail(std::vector<double> &det_err, std::vector<uint8_t> &keep) {
    const aar_tracker_gate_info g = last_gate();
    det_err.assign((size_t)g.n_in, 0.0);
    keep.assign((size_t)g.n_in, 0);
    int32_t n = 0;
    if (aar_tracker_gate_detail(tracker_, &n, det_err.data(), keep.data())) throw std::runtime_error(aar_last_error());
}

LiveTracker::Window LiveTracker::window() {
    int32_t n = 0, has = 0;
    int64_t idx[AAR_TRACKER_MAX_LAG + 1];
    double poses[6 * (AAR_TRACKER_MAX_LAG + 1)], fe[AAR_TRACKER_MAX_LAG + 1], pe[AAR_TRACKER_MAX_LAG + 1], anchor[6];
    if (aar_tracker_window(tracker_, &n, idx, poses, fe, pe, anchor, &has)) throw std::runtime_error(aar_last_error());
    return live_window(n, idx, poses, fe, pe, anchor, has);
}

aar_tracker_uncertainty_record LiveTracker::uncertainty() {
    aar_tracker_uncertainty_record u;
    memset(&u, 0, sizeof u);
    u.struct_size = sizeof u;
    if (aar_tracker_uncertainty(tracker_, &u)) throw std::runtime_error(aar_last_error());
    return u;
}

void LiveTracker::reset() {
    if (aar_tracker_reset(tracker_)) throw std::runtime_error(aar_last_error());
}

// ---- LiveTrackerBank ----
LiveTrackerBank::LiveTrackerBank(const std::vector<const MultiCamMapper *> &solutions, const LiveTracker::Options &o,
                                 const SparseLevMarq<double>::Params *lm) {
    std::vector<const aar_dataset *> ds;
    for (const MultiCamMapper *s : solutions) {
        const aar_dataset *d = s ? s->dataset() : nullptr;
        if (!d) throw std::runtime_error("LiveTrackerBank: member " + std::to_string(ds.size()) + " holds no solution");
        ds.push_back(d);
        cam_index_.emplace_back();
        marker_index_.emplace_back();
        live_index_ids(d, cam_index_.back(), marker_index_.back());
    }
    const aar_tracker_params p = live_params(o);
    const aar_lm_params q = live_lm_params(lm);
    if (aar_tracker_bank_create((int32_t)ds.size(), ds.data(), &p, &q, &bank_)) throw std::runtime_error(aar_last_error());
}

LiveTrackerBank::~LiveTrackerBank() { aar_tracker_bank_destroy(bank_); }

int LiveTrackerBank::size() const { return aar_tracker_bank_size(bank_); }

void LiveTrackerBank::pack(const std::vector<std::vector<LiveTracker::Detection>> &detections, const std::vector<const double *> &starts) {
    const size_t B = cam_index_.size();
    if (detections.size() != B || (!starts.empty() && starts.size() != B)) throw std::runtime_error("LiveTrackerBank: one entry per member is needed");
    n_.clear(); cam_.clear(); marker_.clear(); uv_.clear();
    for (size_t b = 0; b < B; b++) n_.push_back(live_append(cam_index_[b], marker_index_[b], detections[b], cam_, marker_, uv_));
    start_.assign(6 * B, 0.0);
    has_start_.assign(B, 0);
    any_start_ = false;
    for (size_t b = 0; b < starts.size(); b++)
        if (starts[b]) {
            memcpy(&start_[6 * b], starts[b], 6 * sizeof(double));
            has_start_[b] = 1;
            any_start_ = true;
        }
}

std::vector<aar_tracker_result> LiveTrackerBank::push(double frame_time, const std::vector<std::vector<LiveTracker::Detection>> &detections,
                                                      const std::vector<const double *> &starts) {
    pack(detections, starts);
    std::vector<aar_tracker_result> r(cam_index_.size(), blank_result());
    if (aar_tracker_bank_push(bank_, frame_time, n_.data(), cam_.data(), marker_.data(), uv_.data(), any_start_ ? start_.data() : nullptr,
                              any_start_ ? has_start_.data() : nullptr, r.data()))
        throw std::runtime_error(aar_last_error());
    return r;
}

void LiveTrackerBank::enable_detections(const std::vector<LiveTracker::DetectionOptions> &per_member) {
    const size_t B = cam_index_.size();
    if (!per_member.empty() && per_member.size() != B) throw std::runtime_error("LiveTrackerBank::enable_detections: one entry per member, or none");
    std::vector<std::vector<aar_cam_model>> by_index(B);
    std::vector<aar_tracker_detection_params> p(B);
    std::vector<const aar_tracker_detection_params *> ptr(B, nullptr);
    for (size_t b = 0; b < per_member.size(); b++) {
        p[b] = live_detection_params(cam_index_[b], per_member[b], by_index[b], "LiveTrackerBank");
        ptr[b] = &p[b];
    }
    if (aar_tracker_bank_enable_detections(bank_, ptr.data())) throw std::runtime_error(aar_last_error());
}

std::vector<aar_tracker_result> LiveTrackerBank::push_detections(double frame_time, const std::vector<std::vector<LiveTracker::Detection>> &detections,
                                                                 const std::vector<const double *> &starts, std::vector<aar_tracker_start_info> *infos) {
    pack(detections, starts);
    const size_t B = cam_index_.size();
    std::vector<aar_tracker_result> r(B, blank_result());
    if (infos) {
        aar_tracker_start_info si;
        memset(&si, 0, sizeof si);
        si.struct_size = sizeof si;
        infos->assign(B, si);
    }
    if (aar_tracker_bank_push_detections(bank_, frame_time, n_.data(), cam_.data(), marker_.data(), uv_.data(), any_start_ ? start_.data() : nullptr,
                                         any_start_ ? has_start_.data() : nullptr, r.data(), infos ? infos->data() : nullptr))
        throw std::runtime_error(aar_last_error());
    return r;
}

void LiveTrackerBank::enable_gate(const aar_tracker_gate_params *params) {
    aar_tracker_gate_params p;
    aar_tracker_default_gate_params(&p);
    if (aar_tracker_gate_bank_enable(bank_, params ? params : &p)) throw std::runtime_error(aar_last_error());
}

void LiveTrackerBank::enable_motion(const aar_tracker_motion_params *params) {
    aar_tracker_motion_params p;
    aar_tracker_default_motion_params(&p);
    if (aar_tracker_motion_bank_enable(bank_, params ? params : &p)) throw std::runtime_error(aar_last_error());
}

aar_tracker_motion_info LiveTrackerBank::last_motion(int member) {
    aar_tracker_motion_info m;
    memset(&m, 0, sizeof m);
    m.struct_size = (uint32_t)sizeof m;
    if (aar_tracker_motion_bank_last(bank_, member, &m)) throw std::runtime_error(aar_last_error());
    return m;
}

std::array<double, 6> LiveTrackerBank::predict(int member, double time) {
    std::array<double, 6> pose;
    if (aar_tracker_motion_bank_predict(bank_, member, time, pose.data())) throw std::runtime_error(aar_last_error());
    return pose;
}

aar_tracker_gate_info LiveTrackerBank::last_gate(int member) {
    aar_tracker_gate_info g;
    memset(&g, 0, sizeof g);
    g.struct_size = sizeof g;
    if (aar_tracker_gate_bank_last(bank_, member, &g)) throw std::runtime_error(aar_last_error());
    return g;
}

void LiveTrackerBank::gate_detail(int member, std::vector<double> &det_err, std::vector<uint8_t> &keep) {
    const aar_tracker_gate_info g = last_gate(member);
    det_err.assign((size_t)g.n_in, 0.0);
    keep.assign((size_t)g.n_in, 0);
    int32_t n = 0;
    if (aar_tracker_gate_bank_detail(bank_, member, &n, det_err.data(), keep.data())) throw std::runtime_error(aar_last_error());
}

LiveTracker::Window LiveTrackerBank::window(int member) {
    int32_t n = 0, has = 0;
    int64_t idx[AAR_TRACKER_MAX_LAG + 1];
    double poses[6 * (AAR_TRACKER_MAX_LAG + 1)], fe[AAR_TRACKER_MAX_LAG + 1], pe[AAR_TRACKER_MAX_LAG + 1], anchor[6];
    if (aar_tracker_bank_window(bank_, member, &n, idx, poses, fe, pe, anchor, &has)) throw std::runtime_error(aar_last_error());
    return live_window(n, idx, poses, fe, pe, anchor, has);
}

aar_tracker_uncertainty_record LiveTrackerBank::uncertainty(int member) {
    aar_tracker_uncertainty_record u;
    memset(&u, 0, sizeof u);
    u.struct_size = sizeof u;
    if (aar_tracker_bank_uncertainty(bank_, member, &u)) throw std::runtime_error(aar_last_error());
    return u;
}

aar_tracker_bank_stats LiveTrackerBank::stats() const {
    aar_tracker_bank_stats st;
    memset(&st, 0, sizeof st);
    st.struct_size = sizeof st;
    if (aar_tracker_bank_get_stats(bank_, &st)) throw std::runtime_error(aar_last_error());
    return st;
}

void LiveTrackerBank::reset() {
    if (aar_tracker_bank_reset(bank_)) throw std::runtime_error(aar_last_error());
}

bool MultiCamMapper::write_solution_file(std::string path) {
    if (!data_) return false;
    aar_dataset tmp = *data_;
    tmp.optimize_cam_poses = config_.optimize_cam_poses;
    tmp.optimize_marker_poses = config_.optimize_marker_poses;
    tmp.optimize_object_poses = config_.optimize_object_poses;
    tmp.optimize_cam_intrinsics = config_.optimize_cam_intrinsics;
    if (aar_solution_write(path.c_str(), &tmp)) {
        std::cout << aar_last_error() << std::endl;
        return false;
    }
    return true;
}

bool MultiCamMapper::read_solution_file(std::string path) {
    aar_dataset *d = nullptr;
    if (aar_solution_read(path.c_str(), &d)) {
        std::cout << aar_last_error() << std::endl;
        return false;
    }
    drop_problem();
    aar_dataset_free(data_);
    data_ = d;
    cam_models_.clear();
    config_.optimize_cam_poses = d->optimize_cam_poses != 0;
    config_.optimize_marker_poses = d->optimize_marker_poses != 0;
    config_.optimize_object_poses = d->optimize_object_poses != 0;
    config_.optimize_cam_intrinsics = d->optimize_cam_intrinsics != 0;
    mats2eVec();
    return true;
}

void MultiCamMapper::write_text_solution_file(std::string text_path) {
    if (!data_ || aar_solution_write_yaml(text_path.c_str(), data_)) throw std::runtime_error(aar_last_error());
}

static Mat44 to44(const Rigid &T) {
    Mat44 m;
    for (int r = 0; r < 3; r++) {
        for (int c = 0; c < 3; c++) m[r * 4 + c] = T.R[r * 3 + c];
        m[r * 4 + 3] = T.t[r];
    }
    m[12] = m[13] = m[14] = 0;
    m[15] = 1;
    return m;
}

MultiCamMapper::MatArrays MultiCamMapper::get_mat_arrays() {
    MatArrays ma;
    if (!data_) return ma;
    PoseLayout L;
    L.C = data_->num_cams; L.M = data_->num_markers; L.F = data_->num_frames; L.rc = data_->root_cam; L.rm = data_->root_marker;
    for (int c = 0; c < L.C; c++)
        ma.transforms_to_root_cam[data_->cam_ids[c]] = to44(c == L.rc ? Rigid::identity() : pose_to_rigid(data_->x_full + L.full_cam0() + 6LL * L.cam_slot(c)));
    for (int m = 0; m < L.M; m++)
        ma.transforms_to_root_marker[data_->marker_ids[m]] = to44(m == L.rm ? Rigid::identity() : pose_to_rigid(data_->x_full + L.full_mk0() + 6LL * L.mk_slot(m)));
    for (int f = 0; f < L.F; f++) ma.object_to_global[data_->frame_ids[f]] = to44(pose_to_rigid(data_->x_full + L.full_fr0() + 6LL * f));
    return ma;
}

// ---- Initializer mirror (libs/initializer.h) ----
Initializer::Initializer(const aar_detections *dts, double marker_s, const std::vector<aar_cam_model> &cam_c,
                         const std::set<int> &excluded_cs, int device_id) {
    aar_init_params prm;
    aar_init_default_params(&prm);
    prm.marker_size = marker_s;
    prm.device_id = device_id;
    std::vector<int32_t> ex(excluded_cs.begin(), excluded_cs.end());
    prm.n_excluded = (int32_t)ex.size();
    prm.excluded_cams = ex.data();
    if (aar_initializer_run(dts, cam_c.data(), (int32_t)cam_c.size(), &prm, &data_)) throw std::runtime_error(aar_last_error());
}
Initializer::~Initializer() { aar_dataset_free(data_); }
aar_dataset *Initializer::release() {
    aar_dataset *d = data_;
    data_ = nullptr;
    return d;
}
aar_detections *Initializer::read_detections_file(std::string path, const std::vector<int> &subseqs) {
    aar_detections *d = nullptr;
    std::vector<int32_t> ss(subseqs.begin(), subseqs.end());
    if (aar_detections_read(path.c_str(), ss.data(), (int32_t)ss.size(), &d)) throw std::runtime_error(aar_last_error());
    return d;
}
std::set<int> Initializer::get_marker_ids() { return data_ ? std::set<int>(data_->marker_ids, data_->marker_ids + data_->num_markers) : std::set<int>(); }
std::set<int> Initializer::get_cam_ids() { return data_ ? std::set<int>(data_->cam_ids, data_->cam_ids + data_->num_cams) : std::set<int>(); }
int Initializer::get_root_cam() { return data_ ? data_->cam_ids[data_->root_cam] : -1; }
int Initializer::get_root_marker() { return data_ ? data_->marker_ids[data_->root_marker] : -1; }
double Initializer::get_marker_size() { return data_ ? data_->marker_size : 0; }
std::map<int, Mat44> Initializer::get_transforms_to_root_cam() {
    std::map<int, Mat44> r;
    if (!data_) return r;
    PoseLayout L;
    L.C = data_->num_cams; L.M = data_->num_markers; L.F = data_->num_frames; L.rc = data_->root_cam; L.rm = data_->root_marker;
    for (int c = 0; c < L.C; c++)
        r[data_->cam_ids[c]] = to44(c == L.rc ? Rigid::identity() : pose_to_rigid(data_->x_full + L.full_cam0() + 6LL * L.cam_slot(c)));
    return r;
}
std::map<int, Mat44> Initializer::get_transforms_to_root_marker() {
    std::map<int, Mat44> r;
    if (!data_) return r;
    PoseLayout L;
    L.C = data_->num_cams; L.M = data_->num_markers; L.F = data_->num_frames; L.rc = data_->root_cam; L.rm = data_->root_marker;
    for (int m = 0; m < L.M; m++)
        r[data_->marker_ids[m]] = to44(m == L.rm ? Rigid::identity() : pose_to_rigid(data_->x_full + L.full_mk0() + 6LL * L.mk_slot(m)));
    return r;
}
std::map<int, Mat44> Initializer::get_object_transforms() {
    std::map<int, Mat44> r;
    if (!data_) return r;
    PoseLayout L;
    L.C = data_->num_cams; L.M = data_->num_markers; L.F = data_->num_frames; L.rc = data_->root_cam; L.rm = data_->root_marker;
    for (int f = 0; f < L.F; f++) r[data_->frame_ids[f]] = to44(pose_to_rigid(data_->x_full + L.full_fr0() + 6LL * f));
    return r;
}

size_t MultiCamMapper::get_root_cam() { return data_ ? (size_t)data_->cam_ids[data_->root_cam] : 0; }
size_t MultiCamMapper::get_root_marker() { return data_ ? (size_t)data_->marker_ids[data_->root_marker] : 0; }
double MultiCamMapper::get_marker_size() { return data_ ? data_->marker_size : 0; }
void MultiCamMapper::remove_distortions() {
    if (!data_) return;
    aar_dataset *d = data_;
    for (int c = 0; c < d->num_cams; c++) {
        std::vector<int64_t> idx;
        for (int64_t o = 0; o < d->num_obs; o++)
            if (d->obs_cam[o] == c) idx.push_back(o);
        if (idx.empty()) continue;
        std::vector<float> pts(8 * idx.size());
        for (size_t k = 0; k < idx.size(); k++) memcpy(&pts[8 * k], d->obs_uv + 8 * idx[k], 8 * sizeof(float));
        const bool full = (int)cam_models_.size() == d->num_cams;   // built from calibrations: all of distortion_coefficients
        if (aar_undistort_points(d->cam_mats + 9 * c, full ? cam_models_[c].dist : d->dist_coeffs + 5 * c, full ? cam_models_[c].n_dist : 5,
                                 (int64_t)(4 * idx.size()), pts.data(), pts.data(), device_id))
            throw std::runtime_error(aar_last_error());
        for (size_t k = 0; k < idx.size(); k++) memcpy(d->obs_uv + 8 * idx[k], &pts[8 * k], 8 * sizeof(float));
    }
    drop_problem();   // the device copy of the observations is stale now
}

std::vector<std::array<int, 2>> MultiCamMapper::get_image_sizes() {
    std::vector<std::array<int, 2>> r;
    if (data_)
        for (int c = 0; c < data_->num_cams; c++) r.push_back({data_->image_sizes[2 * c], data_->image_sizes[2 * c + 1]});
    return r;
}

}  // namespace aar
