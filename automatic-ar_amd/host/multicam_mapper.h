// Host-side mirror of the reference's MultiCamMapper for the find_solution path
// (libs/multicam_mapper.h:14-83): same method names, argument meaning and error behaviour, with
// cv::Mat replaced by plain 4x4 row-major arrays and Eigen::VectorXd by std::vector<double>, because
// neither OpenCV nor Eigen exists on the GPU box.  Every numeric method forwards to the C ABI of
// include/aar.h (HIP kernels); there is no CPU arithmetic path behind this class.
#pragma once
#include <array>
#include <cstring>
#include <functional>
#include <map>
#include <stdexcept>
#include <type_traits>
#include <utility>
#include <set>
#include <string>
#include <vector>

#include "../../include/aar.h"

namespace aar {

class MultiCamMapper;

// Stand-in for Eigen::SparseMatrix<T> in the signature of a Jacobian function (libs/sparselevmarq.h:63).  The Jacobian of the
// accelerated path never exists as a host matrix -- its blocks are accumulated into J^T J on the device -- so for
// MultiCamMapper's own functions the type only keeps reference-shaped code compiling.  A caller's OWN Jacobian function (the
// host loop of detail::HostLevMarq) fills it entry by entry: coordinate form, duplicates are added up, as Eigen's
// setFromTriplets does.
template <typename T>
struct Triplet {   // Eigen::Triplet's interface
    Triplet() {}
    Triplet(int64_t r, int64_t c, T v) : r_(r), c_(c), v_(v) {}
    int64_t row() const { return r_; }
    int64_t col() const { return c_; }
    T value() const { return v_; }
    int64_t r_ = 0, c_ = 0;
    T v_ = 0;
};
template <typename T>
struct SparseJacobian {
    int64_t rows = 0, cols = 0;
    std::vector<int64_t> row, col;
    std::vector<T> val;
    void resize(int64_t r, int64_t c) { rows = r; cols = c; setZero(); }
    void setZero() { row.clear(); col.clear(); val.clear(); }
    T &insert(int64_t r, int64_t c) { row.push_back(r); col.push_back(c); val.push_back(T(0)); return val.back(); }
    template <class It>
    void setFromTriplets(It begin, It end) { setZero(); for (It t = begin; t != end; ++t) insert(t->row(), t->col()) = t->value(); }
    int64_t nonZeros() const { return (int64_t)val.size(); }
};

namespace detail {
// How the solver mirror recognises the evaluation functions it can run.  The reference's callers hand the solver
// std::bind(&MultiCamMapper::error_function, this, _1, _2) and friends (libs/multicam_mapper.cpp:426,441), which reach the solver
// type-erased.  The mirror calls such a callable ONCE with the probe below raised; the evaluation members of aar::MultiCamMapper
// (error_function, jacobian_function, error_function_tracking) then answer with who they are instead of computing, and the
// solver dispatches to the device path of that mapper (aar_lm_solve / aar_lm_step / aar_track).  A callable that does not
// answer is a host function: the solver throws std::logic_error -- there is no CPU loop behind this class.
enum EvalKind { EVAL_NONE = 0, EVAL_ERROR_FUNCTION = 1, EVAL_JACOBIAN_FUNCTION = 2, EVAL_ERROR_FUNCTION_TRACKING = 3 };
struct EvalId {
    MultiCamMapper *owner = nullptr;
    int kind = EVAL_NONE;
};
struct EvalProbe {
    bool active = false;
    EvalId id;
};
EvalProbe &eval_probe();   // one per thread
// The LM loop of libs/sparselevmarq.h for evaluation functions that live on the host (host_levmarq.cpp): what SparseLevMarq<double> runs when its callables are
// not MultiCamMapper's own.  Dense normal equations, LDL^T without pivoting; same init / step / solve rules, exits and quirks as the reference.
class HostLevMarq {
   public:
    typedef std::vector<double> eVector;
    typedef std::function<void(const eVector &, eVector &)> F;
    typedef std::function<void(const eVector &, SparseJacobian<double> &)> FJ;
    struct Prm {
        int maxIters = 100;
        double minError = 1e-5, min_step_error_diff = 0, min_average_step_error_diff = 0.001, tau = 1, der_epsilon = 1e-3;
        bool verbose = false;
    };
    void init(const eVector &z, const F &f);                                     // libs/sparselevmarq.h:238-249
    bool step(const F &f, const FJ &fJ, const Prm &prm);                         // :349-430
    double solve(eVector &z, const F &f, const FJ &fJ, const Prm &prm, const std::function<void(const eVector &)> &step_cb,
                 const std::function<bool(const eVector &)> &stop_fn);            // :440-472
    static void central_differences(const eVector &z, SparseJacobian<double> &J, const F &f, double der_epsilon);   // :193-214
    eVector curr_z, x;            // current point; the residual vector of the LAST evaluation (the reference's x64)
    double currErr = 0, prevErr = 0, mu = -1, v = 2, last_gain = 0;
    int last_tries = 0, iterations = 0, exit_code = 0;   // exit_code: the reference's mustExit (1 minError, 2 small step / rejected, 3 error grew; 0: maxIters or a stop function)
    bool active = false;          // init() has run on the host path
    SparseJacobian<double> J;
};
// the mapper's device problem (created on demand) and its full parameter vector for the current Config; throws on failure
aar_problem *bind_problem(MultiCamMapper *owner, std::vector<double> &x_full);
aar_problem *current_problem(const MultiCamMapper *owner);   // what the mapper holds right now (nullptr after a Config change)
// MultiCamMapper::track() behind solve(z, error_function_tracking): every frame's own LM on the device; returns the summed final error
double solve_tracking(MultiCamMapper *owner, std::vector<double> &z);
}  // namespace detail

// ucoslam::SparseLevMarq<T> (libs/sparselevmarq.h:26-141) over the C ABI: Params with the reference's field names, setParams,
// solve / init / step with the reference's signatures (:80,88,95-96,118), getCurrentSolution, setStepCallBackFunc, setStopFunction.
// Evaluation functions that are aar::MultiCamMapper's own (see detail::EvalProbe) run on the GPU: error_function + jacobian_function as
// the HIP kernels of that mapper's device problem, error_function_tracking as aar_track; there solve(z, f) -- "automatic Jacobian" in the
// reference, central differences -- uses the same analytic device Jacobian.  Any OTHER callable is a host function: the solver then is the
// reference's general sparse LM on the host (detail::HostLevMarq, host_levmarq.cpp: same rules, exits and quirks; central differences for
// solve(z, f)), as SURVEY.md section 8b keeps it for API compatibility.  The probe costs a host function one extra evaluation per solve / init.
// z is the reference's parameter vector for the problem's Config (mats2eVec order).
template <typename T>
class SparseLevMarq {
    static_assert(std::is_same<T, double>::value, "the accelerated path computes in double, as the reference's instantiation does");

   public:
    struct Params {
        Params() {}
        // (sic) the reference's constructor stores _min_step_error_diff in BOTH step fields (libs/sparselevmarq.h:32-39)
        Params(int _maxIters, T _minError, T _min_step_error_diff = 0, T /*_min_average_step_error_diff*/ = 0.001, T _tau = 1, T _der_epsilon = 1e-3) {
            maxIters = _maxIters;
            minError = _minError;
            min_step_error_diff = _min_step_error_diff;
            min_average_step_error_diff = _min_step_error_diff;
            tau = _tau;
            der_epsilon = _der_epsilon;
        }
        int maxIters = 100;
        T minError = 1e-5;
        T min_step_error_diff = 0;
        T min_average_step_error_diff = 0.001;
        T tau = 1;
        T der_epsilon = 1e-3;  // the host loop's central differences (the device Jacobian is analytic)
        bool cal_dev_parallel = true;
        bool use_omp = true;
        bool verbose = false;
    };
    typedef std::vector<T> eVector;
    typedef std::function<void(const eVector &, eVector &)> F_z_x;
    typedef std::function<void(const eVector &, SparseJacobian<T> &)> F_z_J;

    // the device problem whose kernels stand for f and J; x_full supplies the groups the Config keeps fixed.  The overloads that
    // take the evaluation functions attach by themselves; this is for callers that hold an aar_problem of their own.
    void attach(aar_problem *problem, const double *x_full) {
        problem_ = problem;
        x_.assign(x_full, x_full + aar_problem_full_len(problem));
    }
    void detach() { problem_ = nullptr; }   // the problem is about to be destroyed
    void setParams(int maxIters, T minError, T min_step_error_diff = 0, T tau = 1, T der_epsilon = 1e-3) {   // :259-266
        _params.maxIters = maxIters;
        _params.minError = minError;
        _params.min_step_error_diff = min_step_error_diff;
        _params.tau = tau;
        _params.der_epsilon = der_epsilon;
    }
    void setParams(const Params &p) { _params = p; }

    T solve(eVector &z, F_z_x f_z_x, F_z_J f_J) {   // :80, :440-472
        if (bind_eval(z, f_z_x, &f_J) == detail::EVAL_NONE) return host_.solve(z, f_z_x, f_J, host_prm(), step_cb_, stop_fn_);
        return solve(z);
    }
    T solve(eVector &z, F_z_x f_z_x) {   // :118, :474-477
        const int kind = bind_eval(z, f_z_x, nullptr);
        if (kind == detail::EVAL_NONE) return host_.solve(z, f_z_x, numeric_jacobian(f_z_x), host_prm(), step_cb_, stop_fn_);
        if (kind == detail::EVAL_ERROR_FUNCTION_TRACKING) return detail::solve_tracking(owner_, z);
        return solve(z);
    }
    void init(eVector &z, F_z_x f_z_x) {   // :88, :238-249
        const int kind = bind_eval(z, f_z_x, nullptr);
        if (kind == detail::EVAL_NONE) { host_.init(z, f_z_x); return; }
        if (kind != detail::EVAL_ERROR_FUNCTION) throw std::logic_error("SparseLevMarq::init: the step-by-step mode runs MultiCamMapper::error_function or a host function");
        host_.active = false;
        init(z);
    }
    bool step(F_z_x f_z_x, F_z_J f_J) {   // :95, :349-430
        if (host_.active) return host_.step(f_z_x, f_J, host_prm());   // (the functions init() was given: a host loop cannot tell, the reference does not check either)
        check_eval(f_z_x, &f_J);
        return step();
    }
    bool step(F_z_x f_z_x) {   // :96, :250-256
        if (host_.active) return host_.step(f_z_x, numeric_jacobian(f_z_x), host_prm());
        check_eval(f_z_x, nullptr);
        return step();
    }

    // the same entry points for a problem attached with attach(): no evaluation function to name
    T solve(eVector &z) {   // :440-472
        need();
        install();
        if (aar_problem_merge_z(problem_, z.data(), x_.data())) fail();
        const aar_lm_params p = c_params();
        std::memset(&report, 0, sizeof report);
        if (aar_lm_solve(problem_, x_.data(), &p, &report)) fail();
        if (aar_problem_extract_z(problem_, x_.data(), z.data())) fail();
        return report.final_err;
    }
    void init(eVector &z) {   // :238-249
        need();
        if (aar_problem_merge_z(problem_, z.data(), x_.data())) fail();
        const aar_lm_params p = c_params();
        if (aar_lm_init(problem_, x_.data(), &p)) fail();
    }
    bool step() {   // :349-430; the step callback is solve()'s business in the reference too
        need();
        aar_lm_iter it;
        if (aar_lm_step(problem_, &it)) fail();
        last_iter = it;
        return it.accepted != 0;
    }
    T getCurrentSolution(eVector &z) {   // :432-437
        if (host_.active) { z = host_.curr_z; return host_.currErr; }
        need();
        double err = 0;
        if (aar_lm_get_solution(problem_, x_.data(), &err)) fail();
        z.resize((size_t)aar_problem_num_vars(problem_));
        if (aar_problem_extract_z(problem_, x_.data(), z.data())) fail();
        return err;
    }
    // needs_z = false spares the device -> host copy of curr_z for callbacks that ignore their argument (it is then empty)
    void setStepCallBackFunc(std::function<void(const eVector &)> callback, bool needs_z = true) { step_cb_ = callback; step_needs_z_ = needs_z; }
    void setStopFunction(std::function<bool(const eVector &)> stop_function) { stop_fn_ = stop_function; }

    Params _params;
    aar_lm_report report;     // of the last solve() on the device path
    aar_lm_iter last_iter;    // of the last step() on the device path
    const detail::HostLevMarq &host_state() const { return host_; }   // of the host path: mu, errors, iterations, the reference's exit code

   private:
    void need() const { if (!problem_) throw std::runtime_error("SparseLevMarq: no problem attached"); }
    [[noreturn]] static void fail() { throw std::runtime_error(aar_last_error()); }
    // call the callable once with the probe raised: who is it?
    template <class Fn, class Out>
    static detail::EvalId identify(const Fn &fn, const eVector &z) {
        if (!fn) throw std::logic_error("SparseLevMarq: empty evaluation function");
        detail::EvalProbe &p = detail::eval_probe();
        p.active = true;
        p.id = detail::EvalId();
        Out out;
        try { fn(z, out); } catch (...) { p.active = false; throw; }
        p.active = false;
        return p.id;   // kind EVAL_NONE: nobody answered -- a host function
    }
    static detail::EvalId identify_pair(const eVector &z, const F_z_x &f, const F_z_J *J) {
        const detail::EvalId idf = identify<F_z_x, eVector>(f, z);
        if (idf.kind == detail::EVAL_JACOBIAN_FUNCTION) throw std::logic_error("SparseLevMarq: a Jacobian function was passed as the error function");
        if (J) {
            const detail::EvalId idj = identify<F_z_J, SparseJacobian<T>>(*J, z);
            if (idf.kind == detail::EVAL_NONE && idj.kind == detail::EVAL_NONE) return idf;   // both on the host
            if (idj.kind != detail::EVAL_JACOBIAN_FUNCTION || idj.owner != idf.owner || idf.kind != detail::EVAL_ERROR_FUNCTION)
                throw std::logic_error("SparseLevMarq: error and Jacobian function must be error_function and jacobian_function of the same MultiCamMapper, or both host functions");
        }
        return idf;
    }
    // identify the pair and attach to their mapper's device problem; returns the kind of f
    int bind_eval(const eVector &z, const F_z_x &f, const F_z_J *J) {
        const detail::EvalId id = identify_pair(z, f, J);
        host_.active = false;
        if (id.kind == detail::EVAL_NONE) return id.kind;
        owner_ = id.owner;
        if (id.kind == detail::EVAL_ERROR_FUNCTION) problem_ = detail::bind_problem(owner_, x_);
        return id.kind;
    }
    // step(f, J): the functions must be the ones init() was given
    void check_eval(const F_z_x &f, const F_z_J *J) {
        need();
        const detail::EvalId id = identify_pair(eVector(), f, J);
        if (id.owner != owner_ || id.kind != detail::EVAL_ERROR_FUNCTION) throw std::logic_error("SparseLevMarq::step: not the evaluation functions init() was called with");
        if (detail::current_problem(owner_) != problem_) {   // a Config / data change of the mapper destroyed the problem init() ran on
            problem_ = nullptr;
            throw std::runtime_error("SparseLevMarq::step: the mapper's device problem has changed since init()");
        }
    }
    detail::HostLevMarq::Prm host_prm() const {
        detail::HostLevMarq::Prm p;
        p.maxIters = _params.maxIters; p.minError = _params.minError; p.min_step_error_diff = _params.min_step_error_diff;
        p.min_average_step_error_diff = _params.min_average_step_error_diff; p.tau = _params.tau; p.der_epsilon = _params.der_epsilon; p.verbose = _params.verbose;
        return p;
    }
    F_z_J numeric_jacobian(const F_z_x &f) const {   // libs/sparselevmarq.h:222-228: calcDerivates bound to f
        const double eps = _params.der_epsilon;
        return [f, eps](const eVector &z, SparseJacobian<T> &J) { detail::HostLevMarq::central_differences(z, J, f, eps); };
    }
    aar_lm_params c_params() const {
        aar_lm_params p;
        aar_lm_default_params(&p);
        p.max_iters = _params.maxIters;
        p.min_error = _params.minError;
        p.min_step_error_diff = _params.min_step_error_diff;
        p.min_average_step_error_diff = _params.min_average_step_error_diff;
        p.tau = _params.tau;
        p.verbose = _params.verbose ? 1 : 0;
        return p;
    }
    static void step_tramp(void *ctx, const double *z, int64_t n) {
        SparseLevMarq *self = static_cast<SparseLevMarq *>(ctx);
        if (z) self->zbuf_.assign(z, z + n); else self->zbuf_.clear();
        self->step_cb_(self->zbuf_);
    }
    static int stop_tramp(void *ctx, const double *z, int64_t n) {
        SparseLevMarq *self = static_cast<SparseLevMarq *>(ctx);
        self->zbuf_.assign(z, z + n);
        return self->stop_fn_(self->zbuf_) ? 1 : 0;
    }
    void install() {
        if (aar_lm_set_step_callback(problem_, step_cb_ ? &step_tramp : nullptr, this, step_needs_z_ ? 1 : 0)) fail();
        if (aar_lm_set_stop_function(problem_, stop_fn_ ? &stop_tramp : nullptr, this)) fail();
    }
    aar_problem *problem_ = nullptr;
    detail::HostLevMarq host_;          // the host loop and its state (evaluation functions that are not the mapper's)
    MultiCamMapper *owner_ = nullptr;   // whose evaluation functions the last solve / init named
    std::vector<double> x_;
    eVector zbuf_;
    std::function<void(const eVector &)> step_cb_;
    std::function<bool(const eVector &)> stop_fn_;
    bool step_needs_z_ = true;
};

typedef std::array<double, 16> Mat44;  // row-major 4x4, the reference's CV_64F cv::Mat transforms

// aruco::Marker as the path uses it (3rdparty/aruco/aruco/marker.h:46-58): an id and four image corners x0 y0 .. x3 y3
struct Marker {
    int id = 0;
    float corners[8] = {0, 0, 0, 0, 0, 0, 0, 0};
};
typedef std::map<int, std::map<int, std::vector<Marker>>> FrameCamMarkers;   // frame id -> camera id -> detections, as the reference's fcm

// Mirror of the reference's Initializer (libs/initializer.h:9-43) over aar_initializer_run: the constructor runs
// obtain_pose_estimations + init_transforms (IPPE, candidate sets and votes on the device) and throws std::runtime_error
// on failure; the getters return what the reference's return (ids, id -> 4x4 transform maps).
class Initializer {
   public:
    Initializer(const aar_detections *dts, double marker_s, const std::vector<aar_cam_model> &cam_c,
                const std::set<int> &excluded_cs = std::set<int>(), int device_id = 0);
    ~Initializer();
    Initializer(const Initializer &) = delete;
    Initializer &operator=(const Initializer &) = delete;
    // throws std::runtime_error when the file cannot be opened, as the reference does (libs/initializer.cpp:319-320);
    // free the result with aar_detections_free
    static aar_detections *read_detections_file(std::string path, const std::vector<int> &subseqs = std::vector<int>());
    std::set<int> get_marker_ids();
    std::set<int> get_cam_ids();
    int get_root_cam();
    int get_root_marker();
    std::map<int, Mat44> get_transforms_to_root_cam();
    std::map<int, Mat44> get_transforms_to_root_marker();
    std::map<int, Mat44> get_object_transforms();
    double get_marker_size();
    const aar_dataset *dataset() const { return data_; }
    aar_dataset *release();   // hands the data set to MultiCamMapper(Initializer&)

   private:
    aar_dataset *data_ = nullptr;
};

class MultiCamMapper {
   public:
    typedef SparseLevMarq<double>::eVector eVector;

    struct Config {  // libs/multicam_mapper.h:75-81
        bool optimize_cam_poses = true;
        bool optimize_object_poses = true;
        bool optimize_marker_poses = true;
        bool optimize_cam_intrinsics = true;
    };

    struct MatArrays {  // id -> transform, ascending id (libs/multicam_mapper.h:141-179)
        std::map<int, Mat44> transforms_to_root_cam, transforms_to_root_marker, object_to_global;
    };

    MultiCamMapper();
    // Takes ownership of a data set produced by aar_solution_read / aar_synth_generate: the state the
    // reference's MultiCamMapper(Initializer&) constructor ends with (libs/multicam_mapper.cpp:252-335).
    explicit MultiCamMapper(aar_dataset *dataset);
    explicit MultiCamMapper(Initializer &initializer);   // libs/multicam_mapper.cpp:252-254; takes the initializer's data set
    // libs/multicam_mapper.h:17 / multicam_mapper.cpp:256-259: root ids, id -> 4x4 transform maps (camera -> root camera, marker ->
    // root marker, root marker -> root camera per frame), RAW detections per frame and camera, marker size, calibrations
    // indexed by camera id.  Runs init(): observation order and dropping of unknown cameras / markers as fill_iteration_arrays
    // (:345-377), remove_distortions on the device, "the very initial error" printed -- so it needs a GPU, like the rest.
    MultiCamMapper(size_t root_c, const std::map<int, Mat44> &T_to_root_cam, size_t root_m, const std::map<int, Mat44> &T_to_root_marker,
                   const std::map<int, Mat44> &obj_transforms, const FrameCamMarkers &fcm, float m_size, std::vector<aar_cam_model> &cam_confs);
    void init(size_t root_c, const std::map<int, Mat44> &T_to_root_cam, size_t root_m, const std::map<int, Mat44> &T_to_root_marker,
              const std::map<int, Mat44> &object_poses, const FrameCamMarkers &fcm, float m_size, const std::vector<aar_cam_model> &cam_confs);   // :281-335
    // :272-279, apps/track.cpp:127-131: new frames and RAW detections for a mapper that keeps its cameras, markers and intrinsics
    void init(const std::map<int, Mat44> &object_poses, const FrameCamMarkers &fcm);
    ~MultiCamMapper();
    MultiCamMapper(const MultiCamMapper &) = delete;
    MultiCamMapper &operator=(const MultiCamMapper &) = delete;

    void set_optmize_flag_cam_poses(bool);       // sic: the reference spells it "optmize"
    void set_optmize_flag_marker_poses(bool);
    void set_optmize_flag_object_poses(bool);
    void set_optmize_flag_cam_intrinsics(bool);  // fx cx fy cy (+ the five idle distortion entries) per camera join z (:488-498)
    void set_with_huber(bool);                   // Huber-weighted residual rows + optCallBack's delta schedule (:412-417)
    void set_config(Config &conf);
    size_t get_num_vars(const Config &conf);

    void solve();                                               // libs/multicam_mapper.cpp:419-428
    void track();                                               // :430-443, every frame of the data set at once
    // no counterpart in the reference: track()'s model with a random-walk motion prior between consecutive frames (sigma_rot rad, sigma_trans
    // metre per sqrt(frame id step)), all frames in one LM on the device (aar_track_smooth); the report lands in smooth_report, E_f in
    // track_errors and the pairs' prior costs in smooth_pair_errors
    void track_smooth(double sigma_rot, double sigma_trans);
    // ... under the motion model AAR_SMOOTH_MODEL_* (DESIGN.md section 31).  Constant velocity: sigma_rot / sigma_trans bound the deviation from
    // constant velocity, sigma_rot0 / sigma_trans0 are the sigmas of the first pair's random-walk term; smooth_pair_errors[f] is then term f's cost
    void track_smooth(double sigma_rot, double sigma_trans, int model, double sigma_rot0, double sigma_trans0);
    // EXTENSION, no counterpart in the reference: the pose covariance of the smoothed track at the current poses (aar_track_smooth_covariance,
    // DESIGN.md section 28), with track_smooth()'s prior (the frame ids as its time axis) and Huber delta.  The blocks are UNSCALED: the
    // covariance of frame f is report.sigma2 * frame_cov[f], that of the motion from f to f + 1 follows with lag_cov[f].
    struct SmoothCovariance {
        std::vector<double> frame_cov;   // [num_frames][36] (H^-1)_ff, row-major over (rvec, t)
        std::vector<double> lag_cov;     // [num_frames - 1][36] (H^-1)_{f,f+1}, the rows belong to frame f
        std::vector<double> lag2_cov;    // [num_frames - 2][36] (H^-1)_{f,f+2}, the rows belong to frame f; constant velocity only, else empty
        aar_smooth_covariance_report report = {};
    };
    void track_smooth_covariance(double sigma_rot, double sigma_trans, SmoothCovariance &out);   // throws std::runtime_error on failure
    // ... under the motion model AAR_SMOOTH_MODEL_* with track_smooth()'s sigmas (aar_track_smooth_covariance2): constant
    // velocity adds lag2_cov, with which the covariance of a second difference z_{f+2} - 2 z_{f+1} + z_f follows
    void track_smooth_covariance(double sigma_rot, double sigma_trans, int model, double sigma_rot0, double sigma_trans0,
                                 SmoothCovariance &out);                                          // throws std::runtime_error on failure
    // EXTENSION, no counterpart in the reference: the smoothed track at times that need not be frame times (aar_track_smooth_query, DESIGN.md
    // section 30), with track_smooth()'s prior (the frame ids as its time axis) and Huber delta: what the smoother would report for a frame
    // without detections inserted at each time.  cov is UNSCALED (multiply by report.sigma2) and left empty without covariance.
    struct SmoothQuery {
        std::vector<double> pose;        // [n][6] (rvec, t)
        std::vector<double> cov;         // [n][36] row-major over (rvec, t)
        std::vector<int32_t> segment;    // [n] the frame at or before the time; -1 before the first frame
        aar_smooth_query_report report = {};
    };
    void track_smooth_query(double sigma_rot, double sigma_trans, const std::vector<double> &query_time, SmoothQuery &out,
                            bool covariance = true);                                              // throws std::runtime_error on failure
    // ... under the motion model AAR_SMOOTH_MODEL_* with track_smooth()'s sigmas (aar_track_smooth_query2): under constant
    // velocity the answer is one Gauss-Newton step of the smoother for the inserted frame -- extrapolated outside the recording and across
    // gaps, not held; covariance = false saves the copy of the blocks alone
    void track_smooth_query(double sigma_rot, double sigma_trans, int model, double sigma_rot0, double sigma_trans0,
                            const std::vector<double> &query_time, SmoothQuery &out, bool covariance = true);   // throws std::runtime_error on failure
    // EXTENSION, no counterpart in the reference: the covariance between ANY two frames of the smoothed track and the relative motion between
    // them with its 6x6 covariance (aar_track_smooth_relative), with track_smooth()'s prior (the frame ids as its time axis)
    // and Huber delta, under the motion model AAR_SMOOTH_MODEL_*.  pairs: (a, b) as frame INDICES, any order, duplicates allowed.  The
    // covariances are UNSCALED (multiply by report.sigma2); a velocity over the baseline is rel / dt with rel_cov / dt^2.
    struct SmoothRelative {
        std::vector<double> cross_cov;   // [n][36] (H^-1)_ab, row-major, the rows belong to frame a
        std::vector<double> rel;         // [n][6] [log(R_a^T R_b) ; t_b - t_a]
        std::vector<double> rel_cov;     // [n][36]
        aar_smooth_relative_report report = {};
    };
    void track_smooth_relative(double sigma_rot, double sigma_trans, int model, double sigma_rot0, double sigma_trans0,
                               const std::vector<std::pair<int32_t, int32_t>> &pairs, SmoothRelative &out);   // throws std::runtime_error on failure
    // EXTENSION, no counterpart in the reference: the per-detection layer of the smoothed track at the current poses, with
    // track_smooth()'s prior (the frame ids as its time axis), under the motion model AAR_SMOOTH_MODEL_*.  Everything is UNSCALED (multiply by
    // report.sigma2).  Cameras and markers are named by ID, times are on the frame ids' axis.  All four throw std::runtime_error on failure
    // (std::invalid_argument for an id that does not exist); track_smooth_detection_loo refuses a mapper set_with_huber(true).
    struct SmoothLeverage {
        std::vector<double> leverage, row_leverage;   // [num_obs], [num_obs][8]: trace and diagonal of C_i = G_i (H^-1)_ff G_i^T
        aar_smooth_predict_report report = {};
    };
    void track_smooth_detection_leverage(double sigma_rot, double sigma_trans, int model, double sigma_rot0, double sigma_trans0, SmoothLeverage &out);
    struct SmoothLoo {
        std::vector<double> loo_resid;                // [num_obs][8]
        std::vector<double> q, F, cook, leverage, margin;   // [num_obs]
        std::vector<uint8_t> status, keep;            // [num_obs]; keep = 0 where F > f_max (f_max <= 0: no rule)
        aar_smooth_loo_report report = {};
    };
    void track_smooth_detection_loo(double sigma_rot, double sigma_trans, int model, double sigma_rot0, double sigma_trans0, double f_max,
                                    SmoothLoo &out);
    struct SmoothCorners {
        std::vector<double> uv, cov;                  // [n][8], [n][64] (empty without covariance); the gate: uv = the innovation
        std::vector<double> m2;                       // [n] the gate's e^T (I + C)^-1 e, UNSCALED
        std::vector<uint8_t> status;
        std::vector<int32_t> segment;
        aar_smooth_predict_report report = {};
    };
    void track_smooth_predict_corners(double sigma_rot, double sigma_trans, int model, double sigma_rot0, double sigma_trans0,
                                      const std::vector<int> &cam_ids, const std::vector<int> &marker_ids, const std::vector<double> &times,
                                      SmoothCorners &out, bool covariance = true);
    void track_smooth_gate_detections(double sigma_rot, double sigma_trans, int model, double sigma_rot0, double sigma_trans0,
                                      const std::vector<int> &cam_ids, const std::vector<int> &marker_ids, const std::vector<double> &times,
                                      const std::vector<float> &uv_obs, SmoothCorners &out);
    // ... and the round of -smooth-reject-loo: of every frame the detection with the largest F above f_max is dropped from the data set (the
    // problem is rebuilt on the next use).  Returns the number dropped; out (may be NULL): the report of the call, rejected = that number
    int64_t smooth_reject_loo(double sigma_rot, double sigma_trans, int model, double sigma_rot0, double sigma_trans0, double f_max,
                              SmoothLoo *out = nullptr);
    // EXTENSION, no counterpart in the reference: the corner noise and track_smooth()'s two sigmas fitted to the sequence itself by EM
    // (aar_track_smooth_fit), from the effective start values sigma_rot, sigma_trans.  The frame poses end as the smoothed
    // track at the fitted values; report.sigma_rot_eff / sigma_trans_eff are what track_smooth() and the live tracker take.  A mapper
    // set_with_huber(true) is refused.  fit: NULL = aar_smooth_fit_default_params.
    struct SmoothFit {
        aar_smooth_fit_report report = {};
        std::vector<double> path;        // [report.iterations + 1][3] (sigma_px, sigma_rot, sigma_trans), the start values first
    };
    void fit_smooth_sigmas(double sigma_rot, double sigma_trans, SmoothFit &out, const aar_smooth_fit_params *fit = nullptr);   // throws std::runtime_error on failure
    // ... under the motion model AAR_SMOOTH_MODEL_* (aar_track_smooth_fit2).  Constant velocity: sigma_rot / sigma_trans start
    // the sigmas of the second-difference terms, sigma_rot0 / sigma_trans0 are the first pair's PHYSICAL sigmas and are held: smooth afterwards
    // with report.sigma_rot_eff / sigma_trans_eff and sigma_rot0 / report.sigma_px, sigma_trans0 / report.sigma_px
    void fit_smooth_sigmas(double sigma_rot, double sigma_trans, int model, double sigma_rot0, double sigma_trans0, SmoothFit &out,
                           const aar_smooth_fit_params *fit = nullptr);                            // throws std::runtime_error on failure
    // no counterpart in the reference as a method: apps/track.cpp's loop (:102-136) over the data set's frames, one frame per push through a
    // LiveTracker (below): each frame starts from its own pose in the data set, the frame ids are the time axis; every frame ends at its lagged
    // pose, the last window at aar_tracker_window's.  smooth = false needs lag = 0.  The pushes' results land in live_results.
    // anchor_mode AAR_TRACKER_ANCHOR_MARGINAL (needs smooth and lag >= 1) marginalises the frame that leaves the window instead of freezing it;
    // covariance != NULL also asks for the per-push covariance and receives every frame's lagged block.
    struct LiveCovariance {
        std::vector<double> frame_cov;   // [num_frames][36] the unscaled 6x6 block of H^-1 of the last push that had the frame in its window
        std::vector<double> sigma2;      // [num_frames] that push's sigma2: the pose covariance is sigma2[f] * frame_cov[f]
        std::vector<uint8_t> valid;      // [num_frames] that push's cov_valid
    };
    // gate != NULL gates every pushed frame on the device (aar_tracker_enable_gate); the gate records land in live_gates.
    // motion != NULL gives the tracker a motion model (aar_tracker_enable_motion); the motion records land in live_motions.
    void track_live(int lag, bool smooth, double sigma_rot, double sigma_trans, int anchor_mode = AAR_TRACKER_ANCHOR_FIXED,
                    LiveCovariance *covariance = nullptr, const aar_tracker_gate_params *gate = nullptr,
                    const aar_tracker_motion_params *motion = nullptr);
    // ... the whole of that loop (:117-133): every frame of the data set is fed the RAW detections that carry its frame id (cams: calibrations by
    // camera ID, as the Initializer takes them) and starts from its own vote (start_policy AAR_TRACKER_START_VOTE) or from the cheaper of vote
    // and previous estimate (AAR_TRACKER_START_BEST); the data set's own object poses are not read.  The starts land in live_starts.
    void track_live_from_detections(const aar_detections *detections, const std::vector<aar_cam_model> &cams, int lag, bool smooth, double sigma_rot,
                                    double sigma_trans, int start_policy = AAR_TRACKER_START_VOTE, int anchor_mode = AAR_TRACKER_ANCHOR_FIXED,
                                    LiveCovariance *covariance = nullptr, const aar_tracker_gate_params *gate = nullptr,
                                    const aar_tracker_motion_params *motion = nullptr);
    bool write_live_covariance_file(const std::string &path, const LiveCovariance &cov);   // YAML, aar_tracker_covariance_write_yaml
    void error_function(const eVector &input, eVector &error);  // :731-737
    // :739-801 (private in the reference; public here so that reference-shaped caller code outside the class can bind it).  The
    // Jacobian of the accelerated path is analytic and never leaves the device: called by the solver mirror's probe it names
    // itself (detail::EvalProbe), called directly it throws std::logic_error.
    void jacobian_function(const eVector &input, SparseJacobian<double> &J);
    // :1021-1051, the residual of track(): recognised by SparseLevMarq::solve(z, f) (-> aar_track); a direct call throws
    // std::logic_error (the per-frame residuals of tracking only exist inside k_track)
    void error_function_tracking(const eVector &input, eVector &error);
    void optCallBack(const eVector &v);                         // :412-417
    bool write_solution_file(std::string path);                 // :1053-1099
    bool read_solution_file(std::string path);                  // :1124-1205
    void write_text_solution_file(std::string text_path);       // :1233-1268
    // :554-578: cv::undistortPoints(corners, K, dist, noArray(), P = K) on every detection, camera by camera, on the device.
    // The reference runs it inside init() on raw detections; `.solution` files already hold undistorted corners, so here it is
    // an explicit call for data sets built from raw `aruco.detections` + calib files.  Throws std::runtime_error on failure.
    void remove_distortions();

    MatArrays get_mat_arrays();
    size_t get_root_cam();     // ids, as in the reference
    size_t get_root_marker();
    double get_marker_size();
    std::vector<std::array<int, 2>> get_image_sizes();

    eVector io_vec;           // packed parameters for the current Config (mats2eVec, :445-461)
    float hubberDelta = 2.5;
    SparseLevMarq<double> solver;                 // libs/multicam_mapper.h:198; solve() drives it as the reference does (:419-428)
    SparseLevMarq<double>::Params solver_params;  // what MultiCamMapper::init installs (:326-330)
    aar_lm_report last_report;                    // iterations, errors and timing of the last solve()
    std::vector<int32_t> track_iterations;        // per frame, after track()
    std::vector<double> track_errors;
    aar_smooth_report smooth_report = {};         // after track_smooth()
    std::vector<double> smooth_pair_errors;       // [num_frames - 1] e_f^T L_f e_f, after track_smooth()
    std::vector<aar_tracker_result> live_results; // per frame, after track_live()
    std::vector<aar_tracker_start_info> live_starts;   // per frame, after track_live_from_detections()
    std::vector<aar_tracker_gate_info> live_gates;     // per frame, after track_live() / track_live_from_detections() with a gate
    std::vector<aar_tracker_motion_info> live_motions; // per frame, after track_live() / track_live_from_detections() with a motion model
    int device_id = 0;
    int residual_mode = AAR_RES_F32;
    // How the damped normal equations are solved (aar_solver_options, include/aar.h) -- the counterpart of configuring the reference's solver object
    // through SparseLevMarq::Params (libs/sparselevmarq.h:30-50), and kept beside them.  AUTO (the default) picks by size: the direct chain for one tile of
    // unknowns (<= 16 cameras + markers); CG on the explicit reduced system (SPCG, two-level preconditioned: block-Jacobi + the groups' rigid-motion modes)
    // wherever it fits (<= 224 cameras + markers); CG through the frame blocks (PCG) from 96 entities on when incidences x (incidences per frame - 30) >= 4e6,
    // and where SPCG does not fit -- inexact LM with ONE pose-grade forcing term (SPCG 3e-4, PCG 5e-3) and an absolute tolerance beside it; DIRECT is the
    // reference's Eigen::SimplicialLDLT step to rounding, for callers who want the reference's every step.  Takes effect when the device problem is (re)built: set it before solve() / track();
    // set_solver_options() drops a problem that exists already.
    struct SolverOptions {
        int solver = AAR_SOLVER_AUTO;     // AAR_SOLVER_AUTO | _DIRECT | _SPCG | _PCG
        bool deterministic = false;       // fixed-order sums: two runs give the same bits
        double pcg_eta = 0.0;             // forcing term of the late LM steps (0: the solver's default)
        int pcg_max_it = 0;               // iteration cap of an inner CG solve (0: the solver's default)
        double pcg_eta_loose = 0.0;       // forcing term of the early LM steps (0: default; <= pcg_eta: no sequence)
        double pcg_eta_switch = 0.0;      // "early" = the last accepted step took more than this share of the error away (0: default 0.01)
        double pcg_abs_tol = 0.0;         // absolute tolerance of an inner solve in pose units, beside the relative one (0: default, SPCG 2e-5 / PCG 5e-5)
    };
    void set_solver_options(const SolverOptions &o);
    const SolverOptions &get_solver_options() const { return solver_options_; }
    aar_solver_stats solver_stats();      // what the problem runs with (AUTO resolved) and what its inner solver has done; builds the problem if need be

    // EXTENSION, no counterpart in the reference: the marginal covariance of the current solution (aar_problem_covariance at io_vec's poses,
    // for the current Config).  Blocks are 6x6 row-major over (rx ry rz tx ty tz), SCALED by sigma2, keyed by id as the transforms are;
    // roots, fixed groups and unobserved entities hold NaN.  entity_diag / frame_cov keep the unscaled output of the C call
    // (aar_covariance_write_yaml takes them).  Throws std::runtime_error on failure.
    typedef std::array<double, 36> Mat66;
    struct Covariance {
        double sigma2 = 0;
        aar_covariance_report report{};
        std::map<int, Mat66> cams, markers, objects;   // objects: only when frames were asked for and object poses are optimised
        std::vector<double> entity_diag, frame_cov;
    };
    Covariance compute_covariance(bool frames = true);
    bool write_covariance_file(const std::string &path, const Covariance &cov);   // YAML, aar_covariance_write_yaml

    // EXTENSION, no counterpart in the reference: reprojection errors of the current solution per detection and per camera / marker / frame
    // (aar_problem_residual_report at io_vec's poses, for the current Config); stats are [index][4] {detections, sum r^2, max, rejected} in
    // the data set's index order.  rule NULL: nothing is rejected.  Throws std::runtime_error on failure.
    struct ResidualReport {
        aar_residual_report report{};
        std::vector<double> det_err, cam_stats, marker_stats, frame_stats;
        std::vector<uint8_t> keep;
    };
    ResidualReport residual_report(const aar_outlier_rule *rule = nullptr);
    // drops the detections the rule max(min_px, k_median * median) rejects from the data set and rebuilds the device problem (same Config,
    // solver options and Huber setting) with the current solution as its start; returns how many were dropped (its report in *out if given)
    int64_t reject_outliers(double k_median, double min_px = 0.0, ResidualReport *out = nullptr);
    bool write_residuals_file(const std::string &path, const ResidualReport &rep);   // YAML, aar_residual_report_write_yaml

    // EXTENSION, no counterpart in the reference: where the solved problem expects the four corners of a marker in a
    // camera in a frame, and how well it knows (aar_problem_predict_corners at io_vec's poses, for the current Config).  Queries are by ID:
    // cam_ids[i], marker_ids[i], frame_ids[i]; an unknown id throws std::invalid_argument naming it.  uv [Q][8] = u0 v0 .. u3 v3 in undistorted
    // pixels; cov [Q][64] row-major and SCALED by sigma2 (the a-posteriori covariance of the corners; a NEW detection scatters with
    // cov + sigma2 I); status [Q]: AAR_PREDICT_BEHIND (uv and cov NaN), AAR_PREDICT_UNDEFINED (cov NaN).  covariance = false: uv and status
    // alone, without the covariance chain.  Throws std::runtime_error on failure.
    struct CornerPrediction {
        aar_predict_report report{};
        std::vector<double> uv, cov;
        std::vector<uint8_t> status;
    };
    CornerPrediction predict_corners(const std::vector<int> &cam_ids, const std::vector<int> &marker_ids, const std::vector<int> &frame_ids,
                                     bool covariance = true);
    // the leverage tr(C_i) (0 .. 8, UNSCALED) of every detection of the data set in its order (aar_problem_detection_leverage): a small
    // residual means something only where the leverage is small.  rows: also diag(C_i) [N][8]
    struct DetectionLeverage {
        aar_predict_report report{};
        std::vector<double> leverage, row_leverage;
    };
    DetectionLeverage detection_leverage(bool rows = false);
    // YAML, aar_leverage_write_yaml: det_err as residual_report().det_err, or empty
    bool write_leverage_file(const std::string &path, const DetectionLeverage &lev, double h_min, const std::vector<double> &det_err = {});

    // EXTENSION, no counterpart in the reference: the leave-one-out residual (I - C_i)^-1 r_i of every detection of the
    // data set in its order, the cost q its deletion removes (UNSCALED), the externally studentized F, Cook's distance, leverage, margin,
    // status (AAR_PREDICT_UNDETERMINED: NaN) and keep (0 where F > f_max; f_max <= 0: no rule) -- aar_problem_detection_loo at io_vec's poses.
    // Throws std::runtime_error on failure (a mapper set_with_huber: the statistic rests on the Gaussian model).
    struct DetectionLoo {
        aar_loo_report report{};
        std::vector<double> loo_resid, q, F, cook, leverage, margin;
        std::vector<uint8_t> status, keep;
    };
    DetectionLoo detection_loo(double f_max = 0.0);
    // candidate detections the bundle has not used, by ID as predict_corners; uv [Q][8] observed corners in undistorted pixels.  innovation
    // [Q][8] = observed - predicted, chi2 [Q] = e^T (I + C)^-1 e / sigma2 (ALREADY divided by sigma2: chi-square with 8 degrees of freedom)
    struct GateResult {
        aar_predict_report report{};
        std::vector<double> innovation, chi2;
        std::vector<uint8_t> status;
    };
    GateResult gate_detections(const std::vector<int> &cam_ids, const std::vector<int> &marker_ids, const std::vector<int> &frame_ids,
                               const std::vector<float> &uv);
    // drops, of every frame, the ONE detection with the largest F above f_max (a single-deletion statistic licenses no more) and rebuilds the
    // device problem with the current solution as its start, as reject_outliers does; returns how many were dropped, the report in *out
    // with keep = what was actually dropped
    int64_t reject_loo(double f_max, DetectionLoo *out = nullptr);
    // YAML, aar_loo_write_yaml: det_err as residual_report().det_err, or empty
    bool write_loo_file(const std::string &path, const DetectionLoo &loo, const std::vector<double> &det_err = {});

    // EXTENSION, no counterpart in the reference: per-entity fixing and pose priors (aar_problem_constraints), by ID.
    // Fixed cameras / markers stay exactly where they are; a prior pulls a camera / marker toward a 4x4 transform T (the convention of
    // get_transforms_to_root_cam / _marker) with a 6x6 information matrix over (rx ry rz tx ty tz).  They take effect when the device problem
    // is (re)built and hold across Config changes and reject_outliers rebuilds; a prior on an entity the Config or the fixed sets hold is
    // left out.  An unknown id throws std::invalid_argument when the problem is built (constraint_indices).
    struct PosePrior {
        int kind = AAR_PRIOR_CAMERA;   // AAR_PRIOR_CAMERA | AAR_PRIOR_MARKER
        int id = 0;
        Mat44 T{};
        Mat66 info{};
    };
    // relative pose priors: T is the prior for T_a^-1 T_b of two cameras / two markers given by id (a stereo baseline, a
    // printed board, a bracket).  Held like the pose priors; a pair whose two ends the Config or the fixed sets hold is left out (one held end
    // stays: it is a constant of the term).
    struct RelativePrior {
        int kind = AAR_PRIOR_CAMERA;   // AAR_PRIOR_CAMERA | AAR_PRIOR_MARKER: both ends
        int id_a = 0, id_b = 0;
        Mat44 T{};
        Mat66 info{};
    };
    void set_relative_priors(std::vector<RelativePrior> priors);
    void set_fixed_cams(std::set<int> ids);
    void set_fixed_markers(std::set<int> ids);
    void set_pose_priors(std::vector<PosePrior> priors);
    struct ConstraintIndices {   // what the device problem gets: indices, and the priors as x6 in x_full's convention
        std::vector<int32_t> fixed_cams, fixed_markers;
        std::vector<aar_pose_prior> priors;
        std::vector<aar_pair_prior> pair_priors;
        bool empty() const { return fixed_cams.empty() && fixed_markers.empty() && priors.empty() && pair_priors.empty(); }
    };
    ConstraintIndices constraint_indices() const;
    double prior_cost();   // sum of e^T L e at the current solution (aar_problem_eval_priors); 0 without priors
    double relative_prior_cost();   // the same of the relative priors (aar_problem_eval_pair_priors)

    const aar_dataset *dataset() const { return data_; }

   private:
    friend aar_problem *detail::bind_problem(MultiCamMapper *, std::vector<double> &);
    friend aar_problem *detail::current_problem(const MultiCamMapper *);
    friend double detail::solve_tracking(MultiCamMapper *, std::vector<double> &);
    bool probed(int kind);   // true: the solver mirror asked who this function is (and has been told)
    std::vector<double> problem_vector();
    void mats2eVec();
    void eVec2Mats(const eVector &v);
    int ensure_problem();
    void drop_problem();

    void load_frames(const std::map<int, Mat44> &object_poses, const FrameCamMarkers &fcm);
    aar_dataset *data_ = nullptr;
    aar_problem *problem_ = nullptr;
    std::vector<aar_cam_model> cam_models_;   // per camera INDEX, when the mapper was built from calibrations (full distortion vectors)
    Config config_;
    SolverOptions solver_options_;
    bool with_huber_ = false;
    std::set<int> fixed_cam_ids_, fixed_marker_ids_;
    std::vector<PosePrior> pose_priors_;
    std::vector<RelativePrior> relative_priors_;
};

// EXTENSION, no counterpart in the reference as a class: the live tracker (aar_tracker_*) by camera ID and marker ID.
// Built from a mapper that holds a solution (its cameras, markers and intrinsics; its frames are ignored), then fed one frame per push, in time
// order -- the body of apps/track.cpp's loop (:102-136) without re-initialising anything per frame.  Throws std::runtime_error on failure.
class LiveTracker {
   public:
    struct Detection {
        int cam_id = 0, marker_id = 0;
        float uv[8] = {0, 0, 0, 0, 0, 0, 0, 0};   // undistorted corners x0 y0 .. x3 y3
    };
    struct Options {
        int lag = 0;                  // 0 .. AAR_TRACKER_MAX_LAG
        bool smooth = false;          // false needs lag = 0
        double sigma_rot = 0, sigma_trans = 0;
        bool with_huber = false;
        float huber_delta = 2.5f;
        int max_obs_per_frame = 256;
        int device_id = 0;
        int anchor_mode = AAR_TRACKER_ANCHOR_FIXED;   // AAR_TRACKER_ANCHOR_MARGINAL needs smooth and lag >= 1
        bool covariance = false;                      // every push leaves the window's covariance blocks for uncertainty()
    };
    struct Window {
        std::vector<int64_t> frame_index;
        std::vector<std::array<double, 6>> poses;
        std::vector<double> frame_err, pair_err;   // pair_err[i]: the pair that ends at window frame i (0: the anchor pair)
        bool has_anchor = false;
        std::array<double, 6> anchor_pose{};
    };
    LiveTracker(const MultiCamMapper &solution, const Options &options, const SparseLevMarq<double>::Params *lm = nullptr);
    ~LiveTracker();
    LiveTracker(const LiveTracker &) = delete;
    LiveTracker &operator=(const LiveTracker &) = delete;
    // detections of cameras or markers the solution does not hold are dropped; start: (rvec, t) or NULL = the previous frame's estimate
    aar_tracker_result push(double frame_time, const std::vector<Detection> &detections, const double *start = nullptr);
    // raw detections: once after construction or reset().  cams: calibrations by camera ID (empty: the solution's cam_mats
    // and its five coefficients); then push_detections() takes corners as detected and starts the frame from its own vote (see aar.h)
    struct DetectionOptions {
        std::map<int, aar_cam_model> cams;
        double ippe_threshold = 2.0;
        int min_detections = 2;
        int start_policy = AAR_TRACKER_START_VOTE;
    };
    void enable_detections(const DetectionOptions &options);
    aar_tracker_result push_detections(double frame_time, const std::vector<Detection> &detections, const double *start = nullptr,
                                       aar_tracker_start_info *info = nullptr);
    // the gate: once after construction or reset(), before the first push; NULL = aar_tracker_default_gate_params.  Every
    // pushed frame, plain or raw, then loses the detections the batch path's outlier rule rejects at the pose the push starts from
    void enable_gate(const aar_tracker_gate_params *params = nullptr);
    aar_tracker_gate_info last_gate();                                            // the gate record of the last push
    void gate_detail(std::vector<double> &det_err, std::vector<uint8_t> &keep);   // e_d and keep flags of the newest frame, as pushed to the tracker
    // the motion model: once after construction or reset(), before the first push; NULL = aar_tracker_default_motion_params
    // (constant velocity, no max_dt).  Every pair then carries the motion expected from the two newest estimates, and a frame without a start
    // begins at the prediction
    void enable_motion(const aar_tracker_motion_params *params = nullptr);
    aar_tracker_motion_info last_motion();                                        // the motion record of the last push
    std::array<double, 6> predict(double time);                                   // the newest pose carried to time (host math)
    Window window();
    // aar_tracker_uncertainty: the record of the last push (needs anchor_mode marginal or covariance, and a push since construction / reset)
    aar_tracker_uncertainty_record uncertainty();
    void reset();

   private:
    aar_tracker *tracker_ = nullptr;
    std::map<int, int> cam_index_, marker_index_;
    std::vector<int32_t> cam_, marker_;
    std::vector<float> uv_;
};

// aar_tracker_bank: B live trackers, one per solution, with the same options, advanced in lockstep -- one copy in, one launch of B workgroups and
// one copy out per push.  Every per-member argument is a vector with one entry per member.
class LiveTrackerBank {
   public:
    LiveTrackerBank(const std::vector<const MultiCamMapper *> &solutions, const LiveTracker::Options &options,
                    const SparseLevMarq<double>::Params *lm = nullptr);
    ~LiveTrackerBank();
    LiveTrackerBank(const LiveTrackerBank &) = delete;
    LiveTrackerBank &operator=(const LiveTrackerBank &) = delete;
    int size() const;
    // detections[b]: member b's frame (empty: the object was not seen); starts: empty, or per member (rvec, t) or NULL = its previous estimate
    std::vector<aar_tracker_result> push(double frame_time, const std::vector<std::vector<LiveTracker::Detection>> &detections,
                                         const std::vector<const double *> &starts = {});
    // per_member: empty = the defaults for every member
    void enable_detections(const std::vector<LiveTracker::DetectionOptions> &per_member = {});
    std::vector<aar_tracker_result> push_detections(double frame_time, const std::vector<std::vector<LiveTracker::Detection>> &detections,
                                                    const std::vector<const double *> &starts = {},
                                                    std::vector<aar_tracker_start_info> *infos = nullptr);
    // LiveTracker::enable_gate / last_gate / gate_detail: one parameter set for all members
    void enable_gate(const aar_tracker_gate_params *params = nullptr);
    aar_tracker_gate_info last_gate(int member);
    void gate_detail(int member, std::vector<double> &det_err, std::vector<uint8_t> &keep);
    // LiveTracker::enable_motion / last_motion / predict: one parameter set for all members
    void enable_motion(const aar_tracker_motion_params *params = nullptr);
    aar_tracker_motion_info last_motion(int member);
    std::array<double, 6> predict(int member, double time);
    LiveTracker::Window window(int member);
    aar_tracker_uncertainty_record uncertainty(int member);
    aar_tracker_bank_stats stats() const;
    void reset();

   private:
    void pack(const std::vector<std::vector<LiveTracker::Detection>> &detections, const std::vector<const double *> &starts);
    aar_tracker_bank *bank_ = nullptr;
    std::vector<std::map<int, int>> cam_index_, marker_index_;
    std::vector<int32_t> n_, cam_, marker_;
    std::vector<float> uv_;
    std::vector<double> start_;
    std::vector<uint8_t> has_start_;
    bool any_start_ = false;
};

}  // namespace aar
