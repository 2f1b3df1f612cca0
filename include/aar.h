/*
 * include/aar.h -- C ABI of the MI355X-native sparse-LM bundle-adjustment path.
 *
 * This is the drop-in boundary for ONE path of HSarham/automatic-ar:
 *   MultiCamMapper::solve()  (libs/multicam_mapper.cpp:419-428)
 *     -> ucoslam::SparseLevMarq<double>::solve / init / step  (libs/sparselevmarq.h:440-472,238-249,349-430)
 *     -> MultiCamMapper::error_function / jacobian_function   (libs/multicam_mapper.cpp:731-801)
 * The reference has no FFI of its own (it is one C++ process); the entry points below are what a
 * binding of that path would need, and automatic-ar_amd/host/multicam_mapper.{h,cpp} is the C++ class
 * with the reference's method names that calls them.
 *
 * Conventions: plain pointers and sizes, caller-owned host arrays, no exceptions.  Every function that
 * returns int returns AAR_OK (0) or a negative aar_status; aar_last_error() gives the message of the
 * calling thread's last failure.  All compute entry points run hand-written HIP kernels on gfx950 and
 * FAIL (AAR_ERR_NO_DEVICE) when no GPU is present -- there is no CPU fallback.
 *
 * Pose vectors.  `x_full` is always the reference's default-Config pose vector
 *   [ (C-1) cameras | (M-1) markers | F frames ] x (rx,ry,rz,tx,ty,tz)
 * (fill_io_vec_cams/markers/object_poses, libs/multicam_mapper.cpp:500-522: ascending index, root camera
 * and root marker skipped) i.e. the pose part of the `.solution` vector (:1085-1089).  Which groups are
 * optimised is a flag (MultiCamMapper::Config, libs/multicam_mapper.h:75-81); fixed groups keep their
 * values.  With optimize_cam_intrinsics (off in find_solution, apps/find_solution.cpp:140; on in the reference's default
 * Config) the vectors carry the 9-per-camera intrinsics block behind the poses: see aar_problem_desc.
 */
#ifndef AAR_H
#define AAR_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum aar_status {
    AAR_OK = 0,
    AAR_ERR_INVALID = -1,      /* bad argument / malformed problem                        */
    AAR_ERR_NO_DEVICE = -2,    /* no HIP device: the product has no CPU path              */
    AAR_ERR_HIP = -3,          /* HIP runtime error                                        */
    AAR_ERR_UNSUPPORTED = -4,  /* outside the implemented scope            */
    AAR_ERR_NUMERIC = -5,      /* non-positive pivot in a Cholesky factorisation           */
    AAR_ERR_IO = -6,           /* file could not be opened / short read                    */
    AAR_ERR_COMM = -7          /* RCCL failure                                             */
} aar_status;

const char *aar_last_error(void);

/* ---------------------------------------------------------------------------------------------
 * Data set = everything MultiCamMapper holds after init(): ids, intrinsics, undistorted detections
 * and the pose vector.  Mirrors the content of a `.solution` file (libs/multicam_mapper.cpp:1053-1099).
 * Arrays are owned by the library (free with aar_dataset_free).
 * ------------------------------------------------------------------------------------------- */
typedef struct aar_dataset {
    int32_t num_cams, num_markers, num_frames;
    int32_t root_cam, root_marker;   /* INDICES (rank of the root id in ascending id order)          */
    int32_t *cam_ids;                /* [C] ascending                                                 */
    int32_t *marker_ids;             /* [M] ascending                                                 */
    int32_t *frame_ids;              /* [F] ascending                                                 */
    int32_t *image_sizes;            /* [C][2] width,height                                           */
    double *cam_mats;                /* [C][9] row-major K                                            */
    double *dist_coeffs;             /* [C][5] (carried for the file format; unused by the projection) */
    double marker_size;              /* MultiCamMapper::marker_size: (double)(float)size               */
    int64_t num_obs;                 /* marker observations in reference residual order                */
    int32_t *obs_frame, *obs_cam, *obs_marker; /* [N] indices                                          */
    float *obs_uv;                   /* [N][8] undistorted corners x0 y0 .. x3 y3                       */
    double *x_full;                  /* [6(C-1)+6(M-1)+6F] current pose vector                          */
    double *x_truth;                 /* same layout, ground truth (synthetic data only, else NULL)      */
    int32_t optimize_cam_poses, optimize_marker_poses, optimize_object_poses, optimize_cam_intrinsics;
} aar_dataset;

void aar_dataset_free(aar_dataset *);
int64_t aar_dataset_full_len(const aar_dataset *);   /* 6(C-1)+6(M-1)+6F */

/* Deterministic synthetic multi-camera / multi-marker sequence. */
typedef struct aar_synth_desc {
    int32_t num_cams, num_markers, num_frames;
    uint64_t seed;              /* 20190219 + config index                                             */
    double marker_size;         /* metres (0.05)                                                       */
    double noise_px;            /* corner noise sigma (0.3)                                            */
    double init_rot_sigma;      /* rad, perturbation of every rotation-vector component (0.02)         */
    double init_trans_sigma;    /* m, perturbation of every translation component (0.01)               */
    double init_scale;          /* multiplies both sigmas (1.0)                                        */
    double cam_arc_deg;         /* 0: cameras on a full ring around the scene; > 0: side by side on an arc of that
                                   many degrees centred on camera 0 (config 1, the box-like case: 50)   */
    double min_view_cos;        /* a marker is seen when cos(normal, view ray) >= this (0 = default 0.8;
                                   config 1: 0.35)                                                      */
} aar_synth_desc;
void aar_synth_default(aar_synth_desc *, int32_t config_index); /* BASELINE.json configs[1..4] -> 2..5; 1 = a 3-camera /
                                                                   6-marker stand-in for configs[0] (the box data set) */
int aar_synth_generate(const aar_synth_desc *, aar_dataset **out);

/* File formats of the path.
 *  .solution          libs/multicam_mapper.cpp:1053-1099 (write) / :1124-1205 (read)
 *  .solution.yaml     libs/multicam_mapper.cpp:1233-1268  (cv::FileStorage YAML 1.0 dialect)
 *  aruco.detections   libs/multicam_mapper.cpp:216-237, libs/initializer.cpp:316-348               */
int aar_solution_read(const char *path, aar_dataset **out);
/* flags: AAR_SOLUTION_REFERENCE_INDEXING files the detections as the reference's deserialize_frame_cam_markers does
 * (libs/multicam_mapper.cpp:1101-1122): the f-th frame record under frame id f and the c-th camera record of a frame under
 * camera id c -- the LOOP COUNTERS, not the ids the file stores (:1117-1119).  Same result as the default (ids honoured) when
 * frame / camera ids are 0..n-1 and every frame lists every camera; on `-subseqs` or `-exclude-cams` solutions it is what the
 * reference's track / overlay would see.  A frame counter that is not a stored frame id is AAR_ERR_INVALID. */
#define AAR_SOLUTION_REFERENCE_INDEXING 1
int aar_solution_read_ex(const char *path, int32_t flags, aar_dataset **out);
int aar_solution_write(const char *path, const aar_dataset *);
int aar_solution_write_yaml(const char *path, const aar_dataset *);
int aar_detections_write(const char *path, const aar_dataset *);

/* Camera calibration file <dir>/<cam>/calib.{xml,yml,yaml}: the four keys CamConfig::read_from_file takes from a
 * cv::FileStorage (libs/cam_config.cpp:52-80): image_width, image_height, camera_matrix (3x3), distortion_coefficients
 * (up to AAR_MAX_DIST values in OpenCV's order k1 k2 p1 p2 k3 k4 k5 k6 s1 s2 s3 s4; the rest of dist is zero-filled).
 * XML and YAML 1.0 dialects of cv::FileStorage. */
#define AAR_MAX_DIST 12
int aar_cam_config_read(const char *path, double K[9], double dist[AAR_MAX_DIST], int32_t *n_dist, int32_t *width, int32_t *height);

/* MultiCamMapper::remove_distortions for the corners of ONE camera (libs/multicam_mapper.cpp:554-578):
 * cv::undistortPoints(points, out, K, dist, noArray(), P = K) -- the fixed-point inversion of the distortion model (five
 * iterations, as OpenCV 3.2 does for a coefficient vector) followed by re-projection with K; float in, float out, fp64
 * inside.  Runs on the device (uv_in / uv_out are host pointers, [n_points][2]); uv_out may alias uv_in. */
int aar_undistort_points(const double K[9], const double *dist, int32_t n_dist, int64_t n_points, const float *uv_in,
                         float *uv_out, int32_t device_id);

/* ---------------------------------------------------------------------------------------------
 * Initializer (libs/initializer.cpp): raw detections + calibrations -> the initial solution MultiCamMapper(Initializer&)
 * holds before solve() (apps/find_solution.cpp:118-147).  The pose solver, the candidate sets and the n^2 votes run on the
 * device; the spanning trees (a handful of nodes) on the host.
 * ------------------------------------------------------------------------------------------- */
typedef struct aar_cam_model {       /* CamConfig (libs/cam_config.h)                                          */
    double K[9];                     /* camera_matrix, row-major                                                */
    double dist[AAR_MAX_DIST];       /* distortion_coefficients, OpenCV order, zero-filled                      */
    int32_t n_dist;
    int32_t width, height;
} aar_cam_model;
/* CamConfig::read_cam_configs (libs/cam_config.cpp:80-95): <folder>/<dir>/calib.{xml,yml,yaml} for every sub-directory;
 * camera index = position of the directory in ASCENDING NAME order (the reference takes readdir order).  Free with free(). */
int aar_cam_configs_read(const char *folder, aar_cam_model **out, int32_t *n_cams);
/* dir_order: AAR_DIR_ORDER_NAME (ascending name, "." / ".." skipped: the default above) or AAR_DIR_ORDER_READDIR -- the order
 * readdir lists the sub-directories in, "." and ".." included, exactly as the reference's get_dirs_list (libs/filesystem.cpp:5-17). */
enum { AAR_DIR_ORDER_NAME = 0, AAR_DIR_ORDER_READDIR = 1 };
int aar_cam_configs_read_ex(const char *folder, int32_t dir_order, aar_cam_model **out, int32_t *n_cams);

typedef struct aar_detections {      /* content of an `aruco.detections` file                                   */
    int32_t num_cams;                /* camera slots per frame record                                           */
    int32_t num_frames;              /* frame records                                                           */
    int64_t num_det;
    int32_t *det_frame, *det_cam, *det_id;   /* [num_det], file order: frame, camera slot, detection            */
    float *det_uv;                   /* [num_det][8] RAW (distorted) corners                                    */
} aar_detections;
/* Initializer::read_detections_file (libs/initializer.cpp:316-362).  subseqs = first,last frame pairs
 * (MultiCamMapper::read_subseqs); frames before/between the sub-sequences are emptied, as the reference does. */
int aar_detections_read(const char *path, const int32_t *subseqs, int32_t n_subseqs, aar_detections **out);
void aar_detections_free(aar_detections *);
/* <folder>/subseqs.txt: whitespace-separated frame numbers (libs/multicam_mapper.cpp read_subseqs).  Free with free(). */
int aar_subseqs_read(const char *path, int32_t **out, int32_t *n);

/* aruco::solvePnP_(size, corners, K, dist) (3rdparty/aruco/aruco/ippe.cpp:118-223) for n markers of one camera, on the
 * device: T1 / T2 [n][16] = the two 4x4 marker->camera poses rounded to float as getRTMatrix(.., CV_32F) does, err1 <= err2
 * the float reprojection errors in normalised image units.  uv: [n][8] raw corners (host). */
int aar_ippe_square(double marker_size, const aar_cam_model *cam, int64_t n, const float *uv, double *T1, double *err1,
                    double *T2, double *err2, int32_t device_id);

/* Initializer::find_best_transformation (libs/initializer.cpp:151-193) for n_sets candidate sets at once, on the device.
 * Candidates of set s are [set_begin[s], set_begin[s+1]) of T / T1inv / T2inv ([n][16] row-major 4x4, host).
 * best[s] = index inside the set of the first minimum (-1: empty set), weight[s] = its summed corner distance,
 * cost (optional, [n]) = every candidate's sum. */
int aar_vote_transforms(double marker_size, int64_t n_sets, const int64_t *set_begin, const double *T, const double *T1inv,
                        const double *T2inv, int64_t *best, double *weight, double *cost, int32_t device_id);

typedef struct aar_init_params {
    double marker_size;              /* metres                                                                  */
    double threshold;                /* second IPPE pose kept when err2/err1 < threshold (2.0, initializer.h:52)  */
    int32_t min_detections;          /* frames with fewer detections are dropped (2, initializer.h:51)           */
    int32_t n_excluded;
    const int32_t *excluded_cams;    /* camera slots to ignore (-exclude-cams)                                   */
    int32_t device_id;
} aar_init_params;
void aar_init_default_params(aar_init_params *);
/* Initializer(detections, marker_size, cam_configs, excluded_cams) followed by MultiCamMapper(Initializer&)
 * (libs/initializer.cpp:64-71, libs/multicam_mapper.cpp:252-254,281-331): the data set the reference writes as
 * initial.solution -- ids, intrinsics, corners undistorted with P = K, and the initial pose vector.  cams[i] belongs to
 * camera slot i.  Fails (AAR_ERR_INVALID) when a camera or marker is not connected to the root by co-visibility, where
 * the reference runs into std::map::at. */
int aar_initializer_run(const aar_detections *, const aar_cam_model *cams, int32_t n_cams, const aar_init_params *,
                        aar_dataset **out);
/* The Initializer as apps/track.cpp uses it (:70-89,117-120), for a whole recording at once: the camera and marker
 * transforms of `solution` are GIVEN (set_transforms_to_root_cam / _marker), only obtain_pose_estimations and
 * init_object_transforms run, and the result is what MultiCamMapper::init(object_poses, fcm) holds (libs/multicam_mapper.cpp:
 * 272-279): the solution's cameras / markers / intrinsics, the frames with >= min_detections usable detections, their
 * initial object poses and undistorted corners, optimize flags (0,0,1).  Follow with aar_problem_create + aar_track.
 * Detections of cameras or markers the solution does not hold are dropped. */
int aar_initializer_object_poses(const aar_dataset *solution, const aar_detections *, const aar_cam_model *cams, int32_t n_cams,
                                 const aar_init_params *, aar_dataset **out);

/* cv::Rodrigues as used at libs/multicam_mapper.cpp:470,478 (R row-major 3x3) */
void aar_rodrigues_vec2mat(const double w[3], double R[9]);
void aar_rodrigues_mat2vec(const double R[9], double w[3]);

/* Frame-range partition for `world` ranks, balanced by observation count:
 * rank r owns frames [begin[r], begin[r+1]).  begin has world+1 entries. */
int aar_plan_shards(int32_t num_frames, const int64_t *obs_per_frame, int32_t world, int32_t *begin);

/* ---------------------------------------------------------------------------------------------
 * RCCL communicator (multi-GPU only).  Rank 0 makes an id, the launcher hands it to every rank
 * (bench.py: torch.distributed broadcast), each rank creates its communicator on its own GPU.
 * ------------------------------------------------------------------------------------------- */
typedef struct aar_comm aar_comm;
#define AAR_COMM_ID_BYTES 128
int aar_comm_make_id(char id[AAR_COMM_ID_BYTES]);
int aar_comm_create(const char id[AAR_COMM_ID_BYTES], int32_t world_size, int32_t rank, int32_t device_id,
                    aar_comm **out);
void aar_comm_destroy(aar_comm *);
/* What the communicator has moved so far (bench.py reports it): ranks_seen = ncclCommCount of the RCCL communicator,
 * system_allreduce_bytes = payload of ONE all-reduce of the reduced system (packed lower triangle of S | rhs | g0 | scalars). */
typedef struct aar_comm_stats {
    int32_t world_size, rank, ranks_seen;
    int64_t allreduce_calls, allreduce_bytes, system_allreduce_bytes;
} aar_comm_stats;
int aar_comm_get_stats(const aar_comm *, aar_comm_stats *out);
/* In-process stand-in for a communicator (bring-up and tests on a 1-GPU box): `world_size` host threads of one process,
 * each with its own aar_problem on the same GPU, exchange through the group instead of RCCL; the sharded path itself
 * (frame ranges, every all-reduce, the final gather) is unchanged.  Every rank's calls must be made concurrently, one
 * thread per rank, exactly as separate processes would. */
typedef struct aar_local_group aar_local_group;
int aar_local_group_create(int32_t world_size, aar_local_group **out);
void aar_local_group_destroy(aar_local_group *);
int aar_comm_create_local(aar_local_group *group, int32_t rank, int32_t device_id, aar_comm **out);

/* ---------------------------------------------------------------------------------------------
 * The problem on the device.
 * ------------------------------------------------------------------------------------------- */
typedef struct aar_problem aar_problem;

enum { AAR_RES_F32 = 0,   /* reference-faithful: projection rounded to float, float subtraction
                             (cv::Point2f store + libs/multicam_mapper.cpp:1012-1013)               */
       AAR_RES_F64 = 1 }; /* same formula kept in double                                            */

typedef struct aar_problem_desc {
    int32_t num_cams, num_markers, num_frames;
    int32_t root_cam, root_marker;            /* indices                                            */
    const double *cam_mats;                   /* [C][9]                                             */
    double marker_size;
    int64_t num_obs;
    const int32_t *obs_frame, *obs_cam, *obs_marker;  /* frame-nondecreasing (reference order)      */
    const float *obs_uv;                      /* [N][8]                                             */
    int32_t optimize_cam_poses, optimize_marker_poses, optimize_object_poses;
    int32_t optimize_cam_intrinsics;          /* MultiCamMapper::Config's fourth flag (libs/multicam_mapper.h:75-81): every vector of this
                                                 problem -- x_full, z, delta -- then ENDS with 9 entries per camera, fx cx fy cy d0..d4
                                                 (fill_io_vec_cam_intrinsics, libs/multicam_mapper.cpp:488-498: all cameras, the root too), i.e.
                                                 x_full is the whole `.solution` vector (:1085-1089); cam_mats then only supplies nothing but
                                                 its shape -- the projection uses the pinhole matrix intrinsics_vec2mats rebuilds from those
                                                 four numbers (:580-593, no skew), the five distortion entries are carried along untouched
                                                 (their Jacobian columns are exact zeros in the reference: project_marker ignores them)     */
    int32_t residual_mode;                    /* AAR_RES_F32 | AAR_RES_F64                          */
    int32_t with_huber;                       /* MultiCamMapper::set_with_huber (libs/multicam_mapper.cpp:31-33,1014-1019): residual
                                                 rows scaled by sqrt(rho(e)/e); aar_lm_solve then also runs optCallBack's delta
                                                 schedule (:412-417): 10 at the start of solve(), -7.5/500 per step down to 2.5   */
    int32_t device_id;
    aar_comm *comm;                           /* NULL = single GPU; else observations are sharded by
                                                 frame range over the communicator's ranks           */
} aar_problem_desc;

void aar_problem_desc_from_dataset(const aar_dataset *, aar_problem_desc *);
int aar_problem_create(const aar_problem_desc *, aar_problem **out);   /* = aar_problem_create_ex(desc, NULL, out): solver AUTO */

/* How the damped normal equations of a try are solved -- the counterpart of configuring the reference's solver object through
 * SparseLevMarq::Params / setParams (libs/sparselevmarq.h:30-50,60-66): PER PROBLEM, fixed when the problem is created; two problems
 * of one process may differ.  The reference itself knows one way only (Eigen::SimplicialLDLT, :394-400): AAR_SOLVER_DIRECT is that
 * step to rounding.
 *   AAR_SOLVER_DIRECT  per-frame elimination (Schur complement) + dense blocked LDL^T of the reduced system: the reference's step
 *   AAR_SOLVER_SPCG    the same Schur complement, then block-Jacobi-preconditioned CG on the EXPLICIT reduced system, one wavefront
 *                      per camera / marker (csrc/spcg_kernels.hip), stopped at a relative residual pcg_eta: an inexact LM step.  A solve
 *                      that needs more than pcg_max_it iterations or whose hand-over times out (device shared with another
 *                      process) is redone with the direct chain automatically.  Needs 6 (C + M [+ C]) <= 1344.
 *   AAR_SOLVER_PCG     no Schur complement at all: CG THROUGH the frame blocks (csrc/pcg_kernels.hip); with a communicator the frames'
 *                      blocks stay on their ranks and every CG iteration all-reduces 8 n bytes (nothing O(n^3) is replicated).  At forcing terms
 *                      pcg_eta >= 1e-4 (not deterministic) the frame-entity coupling blocks are kept in fp32 (half the bytes of every CG pass): a rounding
 *                      of 6e-8 there is invisible beside such a forcing term (final poses unchanged: DESIGN.md section 6); tighter terms get fp64 blocks
 *   AAR_SOLVER_AUTO    THE DEFAULT (a NULL options pointer, aar_solver_default_options): the fastest of the three for the problem's size as measured on
 *                      MI355X (profiles/r05_auto_crossover.txt): one tile of unknowns (up to 16 cameras + markers) DIRECT; SPCG wherever
 *                      it fits (up to 224 cameras + markers), except on long sequences whose frames each see many entities, where PCG -- which never
 *                      forms the Schur complement -- overtakes it (from 96 entities on: (entity, frame) incidences x (incidences per frame - 30) >= 4e6, e.g.
 *                      BASELINE.json's 16-camera / 200-marker / 5000-frame configuration); PCG also where SPCG does not fit.
 * Inexact solvers stop an inner solve at a relative residual pcg_eta (PCG: |r| <= eta |b|; SPCG: sqrt(r^T M^-1 r) <= eta sqrt(b^T M^-1 b), M = the
 * block-Jacobi preconditioner).  The LM trajectory is then not the reference's step for step, and -- the reference's stopping rule being loose (its own
 * last step still moves the poses by ~3e-3) -- where a run ends along weakly determined directions depends on every step's accuracy.  The DEFAULT forcing
 * terms (SPCG 3e-4, PCG 5e-3) are therefore chosen for the final POSES: as transforms they agree with the DIRECT solver's to ~2e-6 in the rotation-matrix
 * entries and ~1e-6 m in the translations at BASELINE.json's configurations (tests/test_gpu_solvers.py asserts 1e-5), final reprojection error within
 * 1e-7 px; the direct path itself is ~1e-4 away from the reference-faithful CPU run (analytic against central-difference float Jacobian).
 * pcg_eta_loose > pcg_eta makes a forcing SEQUENCE (pcg_eta_loose while the last accepted LM step still took more than pcg_eta_switch of the error
 * away): faster, and measurably further from the direct run's poses (0.1 -> 0.02, round 4's default: 6e-4) -- opt-in.
 * AAR_SOLVER_DIRECT is the opt-out for callers who want the reference's every step (trace parity).
 * deterministic: every sum the default path leaves to fp64 atomics is taken in a fixed order (as the reference's ascending-row
 * accumulation is, libs/sparselevmarq.h:291-303): two runs give the same bits; slower.
 * Environment variables AAR_SOLVER (direct|spcg|pcg|auto), AAR_DETERMINISTIC, AAR_PCG_ETA, AAR_PCG_MAX_IT apply to problems whose caller
 * left the corresponding field at its default (NULL options, or AUTO / 0): tuning and bisecting only; aar_solver_stats.env_overrides
 * reports what they changed.  An explicitly set field always wins. */
enum { AAR_SOLVER_DIRECT = 0, AAR_SOLVER_PCG = 1, AAR_SOLVER_SPCG = 2, AAR_SOLVER_AUTO = 3 };
typedef struct aar_solver_options {
    uint32_t struct_size;                     /* sizeof(aar_solver_options) of the caller: fields beyond it keep their defaults      */
    int32_t solver;                           /* AAR_SOLVER_*                                                                        */
    int32_t deterministic;                    /* 0 | 1                                                                               */
    int32_t pcg_max_it;                       /* iteration cap of an inner CG solve; 0 = default (PCG 200; SPCG 64 up to four tiles of unknowns,
                                                 128 above -- 128 is also its maximum)                                                */
    double pcg_eta;                           /* forcing term of the inner solves; 0 = default (SPCG 3e-4, PCG 5e-3; aar_solver_stats.pcg_eta reports it)  */
    double pcg_eta_loose;                     /* > pcg_eta: forcing term of the EARLY LM steps (a forcing sequence); 0 = none (default)            */
    double pcg_eta_switch;                    /* an LM step is "early" while the last accepted step took more than this share of the error
                                                 away; 0 = default (0.01)                                                              */
    double pcg_abs_tol;                       /* ABSOLUTE tolerance of an inner solve beside the relative one (both must hold), in the units of the pose
                                                 vector (radians / metres): what the inexact solve may leave out of the step along a weakly determined
                                                 direction, measured in the preconditioner's norm (r^T M^-1 r <= tol^2 mu).  0 = default (SPCG 2e-5, PCG 5e-5); it only binds where the step is large while the damping is small (far
                                                 starts, tau << 1): there the CG runs on, or hands the try to the direct chain at its iteration cap       */
} aar_solver_options;
void aar_solver_default_options(aar_solver_options *);   /* struct_size set, AUTO, not deterministic, default forcing sequence / cap */
int aar_problem_create_ex(const aar_problem_desc *, const aar_solver_options *, aar_problem **out);
/* what the problem runs with (AUTO resolved), and what its inner solver has done so far.  The CALLER sets struct_size = sizeof(aar_solver_stats)
 * before the call; the library fills at most that many bytes, so fields appended LATER do not break a caller built against this layout.
 * ABI note: struct_size itself arrived in round 5, as the FIRST member -- an incompatible change against the round-4 struct (which began with `solver` and
 * carried a `reserved` word): a binary built against round 4 must be rebuilt.  From here on the struct only grows at its end. */
enum { AAR_ENV_SOLVER = 1, AAR_ENV_DETERMINISTIC = 2, AAR_ENV_PCG_ETA = 4, AAR_ENV_PCG_MAX_IT = 8 };
typedef struct aar_solver_stats {
    uint32_t struct_size;                     /* in: sizeof(aar_solver_stats) of the caller                                            */
    int32_t solver;                           /* AAR_SOLVER_DIRECT | _PCG | _SPCG: never AUTO                                         */
    int32_t deterministic;
    int32_t last_iterations;                  /* CG iterations of the last damped solve (0 for DIRECT)                                */
    int64_t total_iterations, solves;         /* since the problem was created                                                        */
    int64_t fallbacks;                        /* SPCG: tries redone with the direct chain (iteration cap, hand-over time-out)          */
    double pcg_eta;                           /* forcing term of the inner solves                                                      */
    int32_t pcg_max_it;
    int32_t env_overrides;                    /* AAR_ENV_* bits: fields an environment variable changed for this problem               */
    int64_t same_xcd_solves;                  /* SPCG: solves whose wavefronts all ran on one XCD (hand-overs through that XCD's L2: the fast case)   */
    double pcg_eta_loose;                     /* forcing term of the early LM steps (0: pcg_eta throughout)                            */
    double pcg_eta_switch;
    double pcg_abs_tol;
} aar_solver_stats;
int aar_problem_get_solver_stats(aar_problem *, aar_solver_stats *out);
/* TESTING ONLY: fault injection for the solvers' fall-back paths.  AAR_TEST_HOOK_SPCG_DROP: the CG wavefront of shared entity `value` never
 * shows up (what a device shared with another process can do): every hand-over times out, the try is redone by the direct chain; -1 clears. */
enum { AAR_TEST_HOOK_SPCG_DROP = 1 };
int aar_problem_set_test_hook(aar_problem *, int32_t hook, int32_t value);
void aar_problem_destroy(aar_problem *);
int64_t aar_problem_full_len(const aar_problem *);    /* length of x_full (+ 9 per camera with optimize_cam_intrinsics) */
int64_t aar_problem_num_vars(const aar_problem *);    /* length of the reference's z for the Config  */
int64_t aar_problem_local_obs(const aar_problem *);   /* observations owned by this rank             */
/* MultiCamMapper::hubberDelta: the delta the next residual evaluations use (only meaningful with with_huber) */
int aar_problem_set_huber_delta(aar_problem *, float delta);
float aar_problem_get_huber_delta(const aar_problem *);

/* error_function (libs/multicam_mapper.cpp:731-737): r (8*num_obs doubles, reference row order; may be
 * NULL; single-GPU only when non-NULL) and sum of squares (all ranks). */
int aar_eval_residuals(aar_problem *, const double *x_full, double *r, double *sum_sq);

/* J^T J and B = -J^T r of libs/sparselevmarq.h:355-367 for the analytic Jacobian, assembled DENSE in the
 * reference's z ordering (P x P row-major, P = aar_problem_num_vars).  For checking the block
 * accumulation kernels on small problems (single GPU).  Either output may be NULL. */
int aar_eval_normal_equations(aar_problem *, const double *x_full, double *JtJ, double *B, double *sum_sq);

/* delta of (J^T J + mu I) delta = B through the device Schur-complement + dense Cholesky path
 * (libs/sparselevmarq.h:384-400), in z ordering. */
int aar_eval_damped_step(aar_problem *, const double *x_full, double mu, double *delta);

/* Covariance of a solved problem (no counterpart in the reference).  (J^T J)^-1 at x_full, UNSCALED -- multiply
 * by sigma2 for the a-posteriori covariance -- in the reference's z ordering for the problem's Config.  Whatever the problem's solver,
 * the normal equations are built with its residual mode and Huber weights, the frames are eliminated at mu = 0 and the reduced system
 * S is factored by the direct chain's LDL^T; S^-1 and the frame marginals V_f^-1 + V_f^-1 W_f^T S^-1 W_f V_f^-1 are formed on the device.
 * Entries of parameters without a z column (roots, non-optimised groups, the five distortion entries of an intrinsics block) and of
 * entities no observation touches are NaN; a frame without observations gets a NaN block.  Any other non-positive pivot of S is
 * AAR_ERR_NUMERIC, naming the entity.  With a communicator S travels in the direct chain's all-reduce, every rank holds the same entity
 * blocks and writes the frame blocks of its own frame range.  Leaves the problem as aar_eval_damped_step does (no LM state).
 *   entity_cov:  Pe x Pe row-major, Pe = num_vars minus the frame-pose unknowns; may be NULL
 *   entity_diag: the diagonal blocks only, z order: 6 x 6 per camera / marker, 9 x 9 per intrinsics entity; may be NULL
 *   frame_cov:   [num_frames][36]: this rank's frames (the others untouched); may be NULL
 *   report:      caller sets struct_size = sizeof(aar_covariance_report); at most that many bytes are filled; may be NULL */
typedef struct aar_covariance_report {
    uint32_t struct_size;
    int64_t num_residuals;                    /* 8 N over all ranks                                                      */
    int64_t num_vars;                         /* P = aar_problem_num_vars                                                */
    double sum_sq;                            /* at x_full, all ranks                                                    */
    double sigma2;                            /* sum_sq / (num_residuals - num_vars): the a-posteriori variance factor   */
    double min_pivot, max_pivot;              /* of D in the LDL^T of S over the rows that carry an unknown (a conditioning hint) */
    int32_t frames_written;                   /* frame blocks this rank wrote                                            */
} aar_covariance_report;
int aar_problem_covariance(aar_problem *, const double *x_full, double *entity_cov, double *entity_diag, double *frame_cov,
                           aar_covariance_report *report);
/* YAML (the cv::FileStorage dialect of aar_solution_write_yaml) of a covariance: per camera id and marker id the 6x6 block
 * sigma2 * entity_diag (rx ry rz tx ty tz) and its 1-sigma rotation (rad) and translation (m) standard deviations; blocks
 * without unknowns (roots, fixed groups, unobserved) as .nan.  entity_diag as aar_problem_covariance writes it for a problem
 * created from `d` (its optimize flags); frame_cov (may be NULL) adds the object poses.  Host code. */
int aar_covariance_write_yaml(const char *path, const aar_dataset *d, const double *entity_diag, const double *frame_cov, double sigma2);

/* Residual report and outlier rejection (no counterpart in the reference).  At x_full, for every detection d (one
 * marker seen by one camera in one frame): e_d = sqrt((sum over its 4 corners of rx^2 + ry^2) / 4) in pixels, summed in fp64 in corner
 * order, UNWEIGHTED (Huber is ignored), with the corner residuals of the problem's residual mode (the rows aar_eval_residuals gives
 * without Huber).  median = the exact lower median of e_d over all ranks (element floor((n-1)/2) of the ascending order), max = the
 * exact maximum; a non-finite e_d sorts above every finite one.  The rule's threshold t = max(min_px, k_median * median) in fp64;
 * k_median <= 0: t = min_px; both <= 0 or no rule: t = +inf.  A detection is kept iff e_d <= t (so a non-finite e_d never is when a
 * rule is given).  Per camera, marker and frame four doubles {detections, sum r^2 over its corners, max e_d, rejected}; an entity
 * without detections gets {0, 0, 0, 0}.  Every output is the same bits from call to call.  With a communicator every rank takes part;
 * median, max, threshold, the keep flags and every count are bit-identical to one GPU, the camera and marker statistics are the same on
 * every rank (and agree with one GPU to rounding).  Leaves the problem as aar_eval_damped_step does (no LM state).
 *   rule:         may be NULL (nothing is rejected but a NaN e_d)
 *   det_err:      [aar_problem_local_obs] e_d of this rank's detections in reference order; may be NULL
 *   keep:         [aar_problem_local_obs] 1 = kept; may be NULL
 *   cam_stats:    [num_cams][4]; marker_stats: [num_markers][4]; may be NULL
 *   frame_stats:  [num_frames][4]: this rank's frames (the others untouched); may be NULL
 *   report:       caller sets struct_size = sizeof(aar_residual_report); required */
typedef struct aar_outlier_rule {
    uint32_t struct_size;                     /* sizeof(aar_outlier_rule)                                                */
    double k_median;                          /* t = max(min_px, k_median * median); <= 0: t = min_px                     */
    double min_px;
} aar_outlier_rule;
typedef struct aar_residual_report {
    uint32_t struct_size;
    int64_t num_detections, num_rejected, num_nonfinite;   /* all ranks                                                      */
    double sum_sq, rmse;                      /* unweighted; rmse = sqrt(sum_sq / (4 num_detections)) per corner coordinate pair */
    double median, max, threshold;            /* threshold = +inf without a rule                                          */
    int32_t cams_emptied, markers_emptied, frames_emptied;   /* had detections, keep none (frames: all ranks)             */
} aar_residual_report;
int aar_problem_residual_report(aar_problem *, const double *x_full, const aar_outlier_rule *rule, double *det_err, uint8_t *keep,
                                double *cam_stats, double *marker_stats, double *frame_stats, aar_residual_report *report);
/* A copy of `d` that keeps the observations with keep[o] != 0, in their order (still frame-nondecreasing).  Every id, camera matrix,
 * x_full, x_truth and the optimize flags are kept; a frame, camera or marker left without detections stays.  Host code. */
int aar_dataset_select_observations(const aar_dataset *d, const uint8_t *keep, aar_dataset **out);
/* YAML (the cv::FileStorage dialect of aar_solution_write_yaml) of a residual report: the report's scalars, per camera id and marker id
 * {detections, rmse, max, rejected} from cam_stats / marker_stats, and the rejected detections as (frame id, camera id, marker id, error)
 * (det_err / keep of a single-GPU report of a problem created from d; both NULL: no list).  Host code. */
int aar_residual_report_write_yaml(const char *path, const aar_dataset *d, const double *cam_stats, const double *marker_stats,
                                   const double *det_err, const uint8_t *keep, const aar_residual_report *report);

/* Predicted marker corners with covariance, and the leverage of every detection (no counterpart in the reference; DESIGN.md section
 * 36).  For a query q = (camera c, marker m, frame f), all three named by INDEX (camera and marker index as in aar_problem_desc, global
 * frame index): u_q = the four projected corners u0 v0 .. u3 v3 at x_full, in the undistorted pixel coordinates the bundle works in,
 * and C_q = G_q Sigma_q G_q^T (8 x 8, row-major, symmetric to the bit) with G_q = du_q / d(camera c, marker m, frame f) (8 x 18) and
 * Sigma_q the 18 x 18 block of (J^T J)^-1 of aar_problem_covariance for that triple, its frame-camera and frame-marker cross blocks
 * included.  C is UNSCALED like everything aar_problem_covariance returns.  HOW TO USE IT: the a-posteriori covariance of a predicted
 * corner is sigma2 * C; the search window for a NEW detection of that marker, whose own pixel noise adds to it, is sigma2 * (C + I).
 * A parameter that is a constant (a root, a member of a non-optimised group, an entity fixed by the caller, the frames of a problem
 * that does not optimise them) contributes ZERO covariance.  status[q]:
 *   bit 0 (AAR_PREDICT_BEHIND):     a corner has non-positive depth in camera c: uv and cov of the query are NaN
 *   bit 1 (AAR_PREDICT_UNDEFINED):  the covariance is undefined: cov is NaN, uv is still written.  This is the case iff frames are optimised
 *                                   and frame f has no observations, or camera c / marker m has a z column, is not held and nothing touches it
 *                                   (the rows aar_problem_covariance reports as NaN because they are unseen)
 * cov == NULL runs no covariance chain: one unpack and one launch give uv and status.  Duplicate queries are allowed; a query's outputs
 * depend on its triple and the solution only, not on the other queries; on a deterministic problem two calls give the same bits.
 * aar_problem_detection_leverage takes the problem's own detections as the queries (reference order, as aar_problem_residual_report):
 * leverage[i] = tr(C_i), between 0 and 8, row_leverage[i][k] = C_i[k][k].  Without priors the leverages sum to num_live_vars and every
 * eigenvalue of C_i lies in [0, 1]: a detection with leverage 8 is contradicted by nothing, and its residual is zero whatever was detected.
 * Refusals, nothing written: a problem with a communicator and a problem created with optimize_cam_intrinsics (its corners also depend on
 * fx, cx, fy, cy: the next step) are AAR_ERR_UNSUPPORTED; whatever makes aar_problem_covariance fail fails here with the same message.
 * Both leave the problem as aar_problem_covariance does (no LM state).  n_query = 0 is AAR_OK and writes nothing but the report.
 *   uv:      [n_query][8];  cov: [n_query][64], may be NULL;  status: [n_query], may be NULL
 *   leverage: [aar_problem_local_obs];  row_leverage: [aar_problem_local_obs][8], may be NULL
 *   report:  caller sets struct_size = sizeof(aar_predict_report); at most that many bytes are filled; may be NULL */
enum { AAR_PREDICT_BEHIND = 1, AAR_PREDICT_UNDEFINED = 2 };
typedef struct aar_predict_report {
    uint32_t struct_size;
    int64_t num_residuals;                    /* 8 N                                                                     */
    int64_t num_vars;                         /* P = aar_problem_num_vars                                                */
    double sum_sq;                            /* at x_full (NaN when no covariance chain ran)                            */
    double sigma2;                            /* sum_sq / (num_residuals - num_vars), as aar_covariance_report           */
    int64_t num_live_vars;                    /* unknowns with a z column that something touches and nobody holds        */
    double leverage_sum;                      /* sum of the finite leverages in detection order (predict_corners: of tr(C_q)) */
    int64_t undefined, behind;                /* queries with status bit 1 / bit 0                                       */
    int32_t launches;                         /* kernel launches of the call                                             */
    double seconds;                           /* wall time of the call                                                   */
} aar_predict_report;
/* Host code, no device: AAR_ERR_INVALID naming the first query whose camera, marker or frame index is out of range (or a NULL array with
 * n_query > 0, or n_query < 0).  n_query = 0 is AAR_OK. */
int aar_predict_query_validate(const aar_problem_desc *, int64_t n_query, const int32_t *q_cam, const int32_t *q_marker, const int32_t *q_frame);
int aar_problem_predict_corners(aar_problem *, const double *x_full, int64_t n_query, const int32_t *q_cam, const int32_t *q_marker,
                                const int32_t *q_frame, double *uv, double *cov, uint8_t *status, aar_predict_report *report);
int aar_problem_detection_leverage(aar_problem *, const double *x_full, double *leverage, double *row_leverage, aar_predict_report *report);
/* YAML (the dialect of aar_residual_report_write_yaml) of the leverages of a single-GPU problem created from d: sigma2, num_live_vars,
 * leverage_sum; per camera id and marker id {detections, mean, max} of the leverages of its detections; the detections with
 * leverage >= h_min (or a non-finite one) as (frame id, camera id, marker id, leverage, error) -- det_err [num_obs] as
 * aar_problem_residual_report gives it, may be NULL (error: .nan).  Host code. */
int aar_leverage_write_yaml(const char *path, const aar_dataset *d, const double *leverage, const double *det_err, double h_min,
                            const aar_predict_report *report);

/* Leave-one-out residuals of every detection, and the gate of candidate detections (no counterpart in the reference; DESIGN.md section
 * 37).  With r_i = observed - u_i (8; the stored float corners widened to double against the projection at x_full, whatever the problem's
 * residual mode) and C_i the 8 x 8 block of aar_problem_detection_leverage, per detection in reference order:
 *   loo_resid[i] = (I - C_i)^-1 r_i     the error detection i would show against a bundle that had not used it
 *   q[i]         = r_i^T (I - C_i)^-1 r_i   the cost that deleting it would remove (unscaled, pixels squared)
 *   F[i]         = (q_i / 8) / ((sum_sq - q_i) / (nu - 8))   the externally studentized statistic, F(8, nu - 8) under the Gaussian model;
 *                  +inf where the denominator is <= 0, NaN where nu <= 8
 *   cook[i]      = w^T C_i w / (num_live_vars sigma2), w = loo_resid[i]   Cook's distance
 *   leverage[i]  = tr(C_i), the bits of aar_problem_detection_leverage
 *   margin[i]    = the smallest pivot met in the Cholesky factorisation of I - C_i (in (0, 1] for a determined detection)
 *   keep[i]      = 0 iff a rule is given, status[i] == 0 and F[i] > rule->f_max; 1 otherwise
 * sum_sq and nu = num_residuals - num_vars are those of the report (predict.sum_sq, dof).  ON A PROBLEM WITH PRIORS sum_sq is what the
 * covariance chain sums: the unweighted squared reprojection residuals PLUS the pose priors' and pair priors' costs, while num_residuals
 * counts the 8 N corner coordinates only and num_vars every z column; F then is the statistic of that convention, not an exact F variate.
 * status[i] carries the bits of aar_problem_predict_corners (NaN outputs) and
 *   bit 2 (AAR_PREDICT_UNDETERMINED): a pivot of I - C_i is <= 1e-6 or not finite -- some direction of the detection's corners is
 *                                     determined by nothing but itself (its frame or its marker has no other detection), so a fit
 *                                     without it does not exist: loo_resid, q, F and cook are NaN, leverage and margin are written, keep = 1.
 * The reading "residual against a fit without the detection" holds to first order at a converged solution (one Gauss-Newton step of the
 * reduced problem from x_full); the quantities themselves are defined as written at any x_full.
 * aar_problem_gate_detections asks the opposite question for CANDIDATE detections the bundle has not used: for query (c, m, f) with
 * observed corners uv_obs (undistorted pixels), innovation = uv_obs - u_q and m2 = e^T (I + C_q)^-1 e, UNSCALED: m2 / sigma2 is chi-square
 * with 8 degrees of freedom under the model.  status as aar_problem_predict_corners (the innovation is still written where only bit 1 is
 * set; m2 is NaN).  The report's leverage_sum is 0.  Queries are validated by aar_predict_query_validate; uv_obs is required when n_query > 0.
 * Both calls run the covariance chain once, leave the problem as aar_problem_covariance does, and write the caller's arrays only after
 * everything succeeded.  Every output array may be NULL.  Refusals, nothing written: all of aar_problem_detection_leverage's;
 * detection_loo on a problem created with_huber is AAR_ERR_UNSUPPORTED (the weights break the Gaussian model the statistic rests on); a
 * rule whose f_max is not positive and finite is AAR_ERR_INVALID.
 *   report.predict: as aar_problem_detection_leverage fills it;  dof = nu;  undetermined / rejected: detections with bit 2 / keep = 0;
 *   f_max: the rule's (+inf without one);  max_f, argmax_f: the largest F that is not NaN and its detection (NaN, -1 when there is none) */
enum { AAR_PREDICT_UNDETERMINED = 4 };
typedef struct aar_loo_rule { uint32_t struct_size; double f_max; } aar_loo_rule;   /* f_max > 0, finite */
typedef struct aar_loo_report {
    uint32_t struct_size;
    aar_predict_report predict;
    int64_t dof;
    int64_t undetermined, rejected;
    double f_max, max_f;
    int64_t argmax_f;
} aar_loo_report;
int aar_problem_detection_loo(aar_problem *, const double *x_full, const aar_loo_rule *rule /* may be NULL */, double *loo_resid /* [N][8] */,
                              double *q /* [N] */, double *F /* [N] */, double *cook /* [N] */, double *leverage /* [N] */,
                              double *margin /* [N] */, uint8_t *status /* [N] */, uint8_t *keep /* [N] */, aar_loo_report *report);
int aar_problem_gate_detections(aar_problem *, const double *x_full, int64_t n_query, const int32_t *q_cam, const int32_t *q_marker,
                                const int32_t *q_frame, const float *uv_obs /* [n][8] */, double *innovation /* [n][8] */,
                                double *m2 /* [n], UNSCALED: chi2_8 = m2 / sigma2 */, uint8_t *status, aar_predict_report *report);
/* YAML (the dialect of aar_leverage_write_yaml) of a leave-one-out report of a single-GPU problem created from d: the report's scalars
 * (sigma2, dof, num_live_vars, f_max, max_f, undetermined, rejected); per camera id and marker id {detections, max_f, rejected} over its
 * detections (max_f over the F that are not NaN, 0 when there is none; rejected = keep is 0); the detections with keep = 0 or an
 * UNDETERMINED status as (frame id, camera id, marker id, F, q, leverage, error).  F, status and keep are required when d has detections;
 * q, leverage and det_err (as aar_problem_residual_report gives it) may be NULL (.nan).  Host code. */
int aar_loo_write_yaml(const char *path, const aar_dataset *d, const double *F, const double *q, const double *leverage, const double *det_err,
                       const uint8_t *status, const uint8_t *keep, const aar_loo_report *report);

/* Per-entity fixing and pose priors (no counterpart in the reference).  Cameras and markers are named by INDEX
 * (problem indices as in aar_problem_desc, not ids).
 *  Fixed entities: fixed_cams / fixed_markers are held where they are, exactly as the roots are.  The layout of z does not change
 *    (num_vars, extract_z, merge_z are those of the problem without constraints); a fixed entity's rows of every step are exactly 0 and
 *    its pose in x_full stays bit-identical.  Naming a root or an entity of a non-optimised group is allowed and changes nothing.
 *    Intrinsics entities are not affected: fixing camera c's pose leaves its intrinsics free.
 *  Pose priors: {kind, index, x6, info}.  x6 is the prior pose as the entity's 6-vector in x_full's convention (rvec, t) -- relative to
 *    the root camera / marker like everything in x_full --, info a symmetric positive semi-definite 6x6 information matrix L (rotation
 *    rows first).  With R, t the entity's current pose the prior residual is
 *        phi = log(R_p^T R)^v,   e = [phi ; t - t_p],   cost = e^T L e
 *    and cost is added to the data's sum r^2 everywhere the solver reads an error (the LM's gain test and stopping rules, aar_lm_report,
 *    aar_eval_normal_equations' sum_sq).  J^T L J (J = [J_r(phi)^-1 J_r(w) 0; 0 I] over the entity's z entries (w, t)) joins the
 *    entity's diagonal block of J^T J and -J^T L e joins B, in every entry point that builds the normal equations: the LM,
 *    aar_eval_normal_equations, aar_eval_damped_step and aar_problem_covariance.  Priors are never Huber-weighted.
 *  Validation (AAR_ERR_INVALID, the message names the entry): an index out of range, two priors on one entity, a prior on a fixed
 *    entity (root, non-optimised group or fixed index), an information matrix that is not symmetric or not positive semi-definite
 *    (a host Cholesky with a negative pivot, or a zero pivot over a non-zero column), a non-finite value.  L = 0 is allowed: it adds
 *    nothing. */
enum { AAR_PRIOR_CAMERA = 0, AAR_PRIOR_MARKER = 1 };
typedef struct aar_pose_prior {
    int32_t kind;                             /* AAR_PRIOR_CAMERA | AAR_PRIOR_MARKER                                      */
    int32_t index;                            /* camera / marker index                                                    */
    double x6[6];                             /* prior pose (rx ry rz tx ty tz), x_full's convention                      */
    double info[36];                          /* row-major 6x6 information matrix, rotation rows first                    */
} aar_pose_prior;
/* Relative pose priors between two cameras or two markers: what a caller who knows a stereo baseline, a printed
 * board layout or a machined bracket knows.  For two entities a != b of the same kind, (R_rel, t_rel) from x6_rel -- the (rvec, t) of
 * T_a^-1 T_b, see aar_relative_pose -- and an information matrix L as in aar_pose_prior (a root's pose is the identity):
 *        R_ab = R_a^T R_b,   t_ab = R_a^T (t_b - t_a),   phi = log(R_rel^T R_ab)^v,   e = [phi ; t_ab - t_rel],   cost = e^T L e
 *    The cost joins the error exactly where the pose priors' does; J_a^T L J_a and J_b^T L J_b join the two entities' diagonal blocks of
 *    J^T J, J_a^T L J_b the block between them, -J^T L e joins B.  Never Huber-weighted; L = 0 adds exact zeros.  An end that is fixed
 *    (root, non-optimised group or fixed index) is a constant of the term: none of its rows, columns or blocks are touched.  Several pairs may
 *    share an entity (a board as a star or a chain), and an entity may carry a pose prior and pair priors together.
 *  Validation (AAR_ERR_INVALID, the message names the entry): an unknown kind, an index out of range, index_a == index_b, the same
 *    unordered pair given twice, both ends fixed, a non-finite value, L not symmetric or not positive semi-definite. */
typedef struct aar_pair_prior {
    int32_t kind;                             /* AAR_PRIOR_CAMERA | AAR_PRIOR_MARKER: both ends are of this kind                 */
    int32_t index_a, index_b;                 /* camera / marker indices                                                  */
    double x6_rel[6];                         /* prior for T_a^-1 T_b as (rx ry rz tx ty tz)                              */
    double info[36];                          /* row-major 6x6 information matrix, rotation rows first                    */
} aar_pair_prior;
typedef struct aar_problem_constraints {
    uint32_t struct_size;                     /* sizeof(aar_problem_constraints) of the caller: fields beyond it count as empty */
    int32_t n_fixed_cams;
    const int32_t *fixed_cams;                /* [n_fixed_cams] camera indices                                            */
    int32_t n_fixed_markers;
    const int32_t *fixed_markers;             /* [n_fixed_markers] marker indices                                         */
    int32_t n_priors;
    const aar_pose_prior *priors;             /* [n_priors]                                                               */
    int32_t n_pair_priors;                    /* (appended: a caller whose struct_size stops before these two has none)   */
    const aar_pair_prior *pair_priors;        /* [n_pair_priors]                                                          */
} aar_problem_constraints;
/* Host function (no device needed): AAR_OK or AAR_ERR_INVALID with a message naming the offending entry.  NULL constraints are valid. */
int aar_problem_constraints_validate(const aar_problem_desc *, const aar_problem_constraints *);
/* aar_problem_create_ex with constraints (validated first).  options may be NULL (AUTO); NULL or empty constraints: exactly
 * aar_problem_create_ex.  With a communicator every rank passes the same constraints; only rank 0 adds the prior terms (the
 * all-reduce of the reduced system makes them global). */
int aar_problem_create_constrained(const aar_problem_desc *, const aar_solver_options *options, const aar_problem_constraints *constraints,
                                   aar_problem **out);
int32_t aar_problem_num_priors(const aar_problem *);
/* The priors at x_full, by the device code the solver runs: e_out [n_priors][6] (may be NULL), cost = sum of e^T L e (may be NULL).
 * With a communicator every rank gets the same values.  Leaves the problem as aar_eval_damped_step does (no LM state). */
int aar_problem_eval_priors(aar_problem *, const double *x_full, double *e_out, double *cost);
int32_t aar_problem_num_pair_priors(const aar_problem *);
/* The pair priors at x_full, by the device code the solver runs: e_out [n_pair_priors][6] (may be NULL), cost = sum of e^T L e (may be NULL).
 * With a communicator every rank gets the same values.  Leaves the problem as aar_eval_damped_step does (no LM state). */
int aar_problem_eval_pair_priors(aar_problem *, const double *x_full, double *e_out, double *cost);
/* x6_rel_out = the (rvec, t) of T_a^-1 T_b for two poses given as (rvec, t): aar_pair_prior.x6_rel of a pair that is where it should be.  Host code. */
int aar_relative_pose(const double *x6_a, const double *x6_b, double *x6_rel_out);

/* ucoslam::SparseLevMarq<T>::Params (libs/sparselevmarq.h:30-50) with the values
 * MultiCamMapper::init installs (libs/multicam_mapper.cpp:326-330). */
typedef struct aar_lm_params {
    int32_t max_iters;                    /* 10000                                                    */
    double min_error;                     /* 1e-5                                                     */
    double min_step_error_diff;           /* 0                                                        */
    double min_average_step_error_diff;   /* 1e-4                                                     */
    double tau;                           /* 1                                                        */
    int32_t verbose;
} aar_lm_params;
void aar_lm_default_params(aar_lm_params *);

typedef struct aar_lm_iter {              /* one step() */
    double err, mu, gain, delta_norm;
    int32_t accepted, tries;
} aar_lm_iter;

typedef struct aar_lm_report {
    int32_t iterations;                   /* step() calls made                                        */
    int32_t stop_code;                    /* mustExit of libs/sparselevmarq.h:458-461 (0 = maxIters)  */
    double initial_err, final_err;        /* sum of squared residuals                                 */
    double final_mu;
    double solve_seconds;                 /* wall time of the loop (device-synchronised)              */
    int64_t trial_points;                 /* residual evaluations inside step()                        */
    aar_lm_iter *trace;                   /* optional caller array                                     */
    int32_t trace_cap;
} aar_lm_report;

/* step-by-step mode: SparseLevMarq::init / step / getCurrentSolution (libs/sparselevmarq.h:238-249,349-437) */
int aar_lm_init(aar_problem *, const double *x_full, const aar_lm_params *);
int aar_lm_step(aar_problem *, aar_lm_iter *out);
int aar_lm_get_solution(aar_problem *, double *x_full, double *err);
/* SparseLevMarq::solve(z, f, J) (libs/sparselevmarq.h:440-472): x_full in/out.  The step callback and the stop function below
 * are honoured exactly where the reference calls them (:446-451, :463). */
int aar_lm_solve(aar_problem *, double *x_full, const aar_lm_params *, aar_lm_report *);

/* The solver seam of ucoslam::SparseLevMarq<T> (libs/sparselevmarq.h:118-123).
 *  setStepCallBackFunc: called on the host after every step() with curr_z -- the reference's z for the problem's Config
 *    (mats2eVec order, aar_problem_num_vars doubles).  want_z = 0 spares the device -> host copy of curr_z for callbacks that
 *    ignore it, as MultiCamMapper::optCallBack does (libs/multicam_mapper.cpp:412-417); z is then NULL.
 *  setStopFunction: when set, solve() runs do { step(); callback; } while (!stop(curr_z)) with NO iteration cap and none of the
 *    error-based exits (:444-450); nonzero = stop.
 * NULL clears.  A with_huber problem without a step callback runs the mapper's own pair -- hubberDelta = 10 at the start of
 * solve(), optCallBack's schedule per step; a caller that installs a callback owns both (aar_problem_set_huber_delta).
 * On a sharded problem every rank must install the same kind of callback (fetching curr_z is a collective). */
typedef void (*aar_lm_step_callback)(void *ctx, const double *z, int64_t num_vars);
typedef int (*aar_lm_stop_function)(void *ctx, const double *z, int64_t num_vars);
int aar_lm_set_step_callback(aar_problem *, aar_lm_step_callback fn, void *ctx, int32_t want_z);
int aar_lm_set_stop_function(aar_problem *, aar_lm_stop_function fn, void *ctx);
/* z <-> x_full for the problem's Config (mats2eVec / eVec2Mats, libs/multicam_mapper.cpp:445-461,595-606): extract copies the
 * optimised groups of x_full into z; merge writes z back into x_full and leaves the fixed groups alone. */
int aar_problem_extract_z(const aar_problem *, const double *x_full, double *z);
int aar_problem_merge_z(const aar_problem *, const double *z, double *x_full);

/* MultiCamMapper::track() (libs/multicam_mapper.cpp:430-443) for every frame of the problem at once: cameras and markers
 * stay at their x_full values, each frame's object pose is refined on its own by the LM of SparseLevMarq::solve(z, f)
 * (libs/sparselevmarq.h:223-228) over error_function_tracking (libs/multicam_mapper.cpp:678-729: double residuals, Huber
 * weights with the problem's current delta when with_huber).  The whole loop of a frame runs on the device.
 * iterations / final_err: optional [num_frames] outputs (step() calls made, final sum of squares per frame). */
int aar_track(aar_problem *, double *x_full, const aar_lm_params *, int32_t *iterations, double *final_err);

/* Smoothed tracking (no counterpart in the reference): aar_track's model with a motion prior between consecutive frames,
 * solved as ONE Levenberg-Marquardt problem over all 6 num_frames frame unknowns on the device.  Cameras, markers and intrinsics stay at
 * their x_full values and the optimize_* flags are ignored, exactly as in aar_track.
 *     E(z) = sum_f E_f(z_f) + sum_{f < F-1} e_f^T L_f e_f
 *     e_f  = [ log((R_f dR_f)^T R_{f+1})^v ; t_{f+1} - t_f - dt_f ],   L_f = diag(1 / (sigma_rot^2 D_f) x3, 1 / (sigma_trans^2 D_f) x3)
 *  E_f is aar_track's frame error (double residuals, Huber weights with the problem's current delta when with_huber); the prior is never
 *  Huber-weighted.  D_f = frame_time[f+1] - frame_time[f] (1 when frame_time is NULL): pass frame ids or time stamps, so that a hole in the
 *  recording is bridged more loosely than one frame step.  (dR_f, dt_f) = rel_motion[f] as (rvec, t), the expected motion from f to f+1
 *  (NULL: none, a random walk on the pose); feeding the relative motions of a previous pass gives constant-velocity behaviour.
 *  The LM is SparseLevMarq's (mu_0 = tau max diag H, the gain test, mu *= v / v *= 5 with at most five retries, exits 1 / 2 / 3 with
 *  rows = 8 num_obs + 6 (num_frames - 1)); every try solves the block-tridiagonal (H + mu I) delta = b by block cyclic reduction.  A frame
 *  without detections is carried by its neighbours.  Results are bit-reproducible from call to call.
 *  Structs are size-versioned: the caller sets struct_size, fields beyond it read as NULL / are not written.
 *  On a problem with a communicator both calls return AAR_ERR_UNSUPPORTED on every rank (the chain crosses shard boundaries).  Leaves no
 *  LM state behind (as aar_track). */
typedef struct aar_smooth_params {
    uint32_t struct_size;
    double sigma_rot;            /* rad   per sqrt(unit of frame_time), > 0 finite */
    double sigma_trans;          /* metre per sqrt(unit of frame_time), > 0 finite */
    const double *frame_time;    /* [num_frames] strictly ascending, finite; NULL = 0,1,2,... */
    const double *rel_motion;    /* [num_frames-1][6] expected (rvec, t) from f to f+1; NULL = none */
    int32_t model;               /* AAR_SMOOTH_MODEL_*; a struct that ends before it reads as AAR_SMOOTH_MODEL_RANDOM_WALK */
    double sigma_rot0;           /* constant velocity only: the sigmas of pair 0, the prior on the first velocity; > 0 finite */
    double sigma_trans0;
} aar_smooth_params;
/* The motion model of the prior.
 *  AAR_SMOOTH_MODEL_RANDOM_WALK: the prior above, bit for bit what a struct without the field gives.
 *  AAR_SMOOTH_MODEL_CONSTANT_VELOCITY: a second-difference prior, the joint minimiser and not a previous pass fed back.  With
 *  between(z_a, z_b, rel) = [ log((R_a dR)^T R_b)^v ; t_b - t_a - dt ] and L(sr, st, D) = diag(1 / (sr^2 D) x3, 1 / (st^2 D) x3):
 *     pair 0   e_0 = between(z_0, z_1) with L(sigma_rot0, sigma_trans0, D_0): the prior on the first velocity, which makes H positive definite
 *              exactly where the random walk's is
 *     term f   (1 <= f <= num_frames - 2)  e_f = between(z_f, z_{f+1}, rel_f),  rel_f = r_f between(z_{f-1}, z_f),  r_f = D_f / D_{f-1}:
 *              dR_f = Exp(r_f log(R_{f-1}^T R_f)),  dt_f = r_f (t_f - t_{f-1}),  with L(sigma_rot, sigma_trans, D_f)
 *  so sigma_rot / sigma_trans bound the deviation from constant velocity per sqrt(unit of frame_time).  The expected motion is a function of
 *  the unknowns and the full Jacobian is used; H is block pentadiagonal and every try solves it by the cyclic reduction on pairs of frames
 *  (12x12 blocks).  rows = 8 num_obs + 6 (num_frames - 1) as before; pair_err[0] is pair 0, pair_err[f] term f.  rel_motion must be NULL
 *  (AAR_ERR_INVALID).  aar_track_smooth, aar_track_smooth_system2, aar_track_smooth_covariance2, aar_track_smooth_fit2,
 *  aar_track_smooth_fit_terms2 and aar_track_smooth_query2 honour the model; aar_track_smooth_system, _covariance, _fit, _fit_terms and _query
 *  return AAR_ERR_UNSUPPORTED under constant velocity and write nothing (their selected inverse is the tridiagonal one). */
#define AAR_SMOOTH_MODEL_RANDOM_WALK 0
#define AAR_SMOOTH_MODEL_CONSTANT_VELOCITY 1
typedef struct aar_smooth_report {
    uint32_t struct_size;
    int32_t iterations, stop_code, rejected_tries;
    double initial_cost, final_cost, final_data_cost, final_prior_cost, final_mu, seconds;
} aar_smooth_report;
/* Host function (no device needed): AAR_OK or AAR_ERR_INVALID with a message naming the sigma or the index in frame_time / rel_motion. */
int aar_smooth_params_validate(int32_t num_frames, const aar_smooth_params *);
/* x_full in/out (only the frame poses move).  NULL aar_lm_params: the defaults.  frame_err [num_frames]: E_f at the result, pair_err
 * [num_frames-1]: e_f^T L_f e_f at the result, report: each may be NULL. */
int aar_track_smooth(aar_problem *, double *x_full, const aar_lm_params *, const aar_smooth_params *, double *frame_err, double *pair_err,
                     aar_smooth_report *report);
/* The system of one try at x_full, for checking: diag [num_frames][36] = H_ff, off [num_frames-1][36] = H_{f,f+1} (row-major, rows: frame f),
 * rhs [6 num_frames] = b, delta [6 num_frames] = the solution of (H + mu I) delta = b by the device's reduction (AAR_ERR_NUMERIC on a
 * non-positive pivot), cost = {sum_f E_f, sum_f e_f^T L_f e_f}.  Every output may be NULL. */
int aar_track_smooth_system(aar_problem *, const double *x_full, const aar_smooth_params *, double mu, double *diag, double *off, double *rhs,
                            double *delta, double cost[2]);
/* The same for either model: off2 [num_frames-2][36] = H_{f,f+2} (row-major, rows: frame f), zeros under the random walk; delta by the
 * reduction of the model in aar_smooth_params. */
int aar_track_smooth_system2(aar_problem *, const double *x_full, const aar_smooth_params *, double mu, double *diag, double *off, double *off2,
                             double *rhs, double *delta, double cost[2]);
/* Host function: the kernel launches of ONE damped solve inside aar_track_smooth / aar_track_smooth_system(2) at this size under the model
 * (AAR_SMOOTH_MODEL_*): one launch while the whole reduction fits the workgroup that finishes it, else 2 + 2 per level launched on its own. */
int32_t aar_smooth_solve_launches(int32_t num_frames, int32_t model);
/* Pose covariance of the smoothed track: the selected inverse of the H that aar_track_smooth_system returns at mu = 0 for
 * the same x_full and parameters (data blocks with the problem's Huber weights, prior blocks with frame_time and rel_motion).
 *   frame_cov [num_frames][36]   = (H^-1)_ff,      row-major over (rvec, t), symmetric to the bit
 *   lag_cov   [num_frames-1][36] = (H^-1)_{f,f+1}, row-major, the rows belong to frame f; it makes the uncertainty of a relative motion
 *                                  computable: Cov(z_{f+1} - z_f) = S_ff + S_{f+1,f+1} - S_{f,f+1} - S_{f,f+1}^T
 * Both are UNSCALED (the convention of aar_problem_covariance and aar_tracker_uncertainty): multiply by report->sigma2.  Computed on the
 * device from what the solve's cyclic reduction keeps, by one pass back down its elimination tree; bit-reproducible from call to call.
 * x_full is not modified; no LM state is left behind.  frame_cov, lag_cov and report may each be NULL.  num_frames = 0: AAR_OK, nothing
 * written; num_frames = 1: frame_cov[0] = V_0^-1.  A frame without detections gets an ordinary finite block as long as the chain of priors
 * ties it to an observed frame.  A non-positive pivot returns AAR_ERR_NUMERIC and writes nothing; the root pivot counts as non-positive when
 * it is not above 64 eps times the largest diagonal entry of H_00, the rounding level of its own computation (the extreme case: no detection
 * in any frame, the prior alone is singular).  A problem with a communicator: AAR_ERR_UNSUPPORTED on every rank. */
typedef struct aar_smooth_covariance_report {
    uint32_t struct_size;
    int64_t num_residuals;       /* 8 num_obs + 6 (num_frames - 1) */
    int64_t num_vars;            /* 6 num_frames */
    double data_cost, prior_cost;
    double sigma2;               /* (data_cost + prior_cost) / (num_residuals - num_vars), 0 when that is <= 0 */
    int32_t launches;
    double seconds;
} aar_smooth_covariance_report;
int aar_track_smooth_covariance(aar_problem *, const double *x_full, const aar_smooth_params *, double *frame_cov, double *lag_cov,
                                aar_smooth_covariance_report *report);
/* The same for either model, with the lag-two blocks that the block-pentadiagonal H of constant velocity brings:
 *   lag2_cov [num_frames-2][36] = (H^-1)_{f,f+2}, row-major, the rows belong to frame f.  With it the covariance of a second difference,
 *                                 the quantity the constant-velocity prior constrains, is computable from the three outputs.
 * AAR_SMOOTH_MODEL_CONSTANT_VELOCITY: H is what aar_track_smooth_system2 returns at mu = 0 for the same inputs; frame_cov, lag_cov and lag2_cov
 * are UNSCALED and the report is that of aar_track_smooth_covariance.  One pass back down the elimination tree of the solve's cyclic reduction
 * on pairs of frames (12x12 blocks); bit-reproducible, frame_cov symmetric to the bit, x_full not modified, no LM state left behind.  Each
 * output and the report may be NULL.  num_frames = 0: AAR_OK, nothing written; 1: frame_cov[0] = V_0^-1; 2: pair 0 alone.  AAR_ERR_NUMERIC
 * with nothing written on a non-positive pivot; the root's pivots count as non-positive when not above 64 eps times the largest diagonal
 * entry of H_00 and H_11 (no detection in any frame: the prior alone is singular).  Huber problems are accepted; a problem with a
 * communicator is AAR_ERR_UNSUPPORTED.
 * AAR_SMOOTH_MODEL_RANDOM_WALK: aar_track_smooth_covariance itself, the same bits; lag2_cov != NULL is AAR_ERR_UNSUPPORTED with nothing
 * written (the tridiagonal selected inverse does not contain that block).
 * aar_track_smooth_covariance, _fit, _fit_terms and _query keep returning AAR_ERR_UNSUPPORTED under constant velocity (the fit under that
 * model is aar_track_smooth_fit2, the track at any time aar_track_smooth_query2). */
int aar_track_smooth_covariance2(aar_problem *, const double *x_full, const aar_smooth_params *, double *frame_cov, double *lag_cov,
                                 double *lag2_cov, aar_smooth_covariance_report *report);
/* Fitting the smoother's noise levels from the recorded sequence itself: expectation-maximisation over
 *   sigma_px (the corner noise the data term fixes at 1 px), sigma_rot, sigma_trans (per sqrt(unit of frame_time)).
 * Only the ratios sigma / sigma_px enter aar_track_smooth's estimate: it is run at the EFFECTIVE sigmas sigma_rot / sigma_px and
 * sigma_trans / sigma_px.  One iteration: aar_track_smooth from the previous track at the current effective sigmas; H at mu = 0, its elimination
 * and the blocks of aar_track_smooth_covariance, all kept on the device; per pair f (g = f + 1, D_f as above, phi, e_t, M_a, M_b of the
 * between factor at the track)
 *   a_r = |phi|^2 / D_f,  u_r = tr(M_a S_ff^ww M_a^T + M_b S_gg^ww M_b^T + M_a S_fg^ww M_b^T + M_b S_fg^ww^T M_a^T) / D_f
 *   a_t = |e_t|^2 / D_f,  u_t = tr(S_ff^tt + S_gg^tt - S_fg^tt - S_fg^tt^T) / D_f         (^ww, ^tt: rotation / translation 3x3 sub-blocks)
 * summed to A_r, U_r, A_t, U_t in a fixed order, U_d = 6 num_frames - U_r / sigma_rot_eff^2 - U_t / sigma_trans_eff^2 (= sum_f tr(V_f S_ff)),
 * and with q = sigma_px^2
 *   sigma_rot^2 <- (A_r + q U_r) / (3 (num_frames - 1)),  sigma_trans^2 <- (A_t + q U_t) / (3 (num_frames - 1)),
 *   q <- (data_cost + q U_d) / (8 num_obs),               all three from the old q.
 * It stops when the largest relative change of an estimated sigma is below rel_tol (stop_code 1) or after max_iters iterations (2), and ends
 * with one aar_track_smooth at the fitted values: x_full (in/out, only the frame poses move) is the track at those.
 * aar_smooth_params: sigma_rot, sigma_trans are the effective start values (sigma_px starts at 1); frame_time and rel_motion are kept.
 * estimate_* = 0 holds that sigma at its start value; estimate_px = 0 fits the effective sigmas directly (sigma_px = 1 exactly).
 * path: NULL or [max_iters + 1][3] = (sigma_px, sigma_rot, sigma_trans) at the start and after every iteration (rows beyond
 * report->iterations are not written).  NULL aar_lm_params / aar_smooth_fit_params: the defaults.  Bit-reproducible from call to call.
 * AAR_ERR_INVALID: num_frames < 2, no detections, all estimate_* zero, rel_tol negative or not finite, max_iters < 1.  AAR_ERR_UNSUPPORTED: a
 * problem created with_huber (the weights break the Gaussian data model), a communicator.  AAR_ERR_NUMERIC: a non-positive pivot, an M-step
 * that gives a variance that is not positive and finite.  On an error nothing is written: x_full, path and report keep their contents. */
typedef struct aar_smooth_fit_params {
    uint32_t struct_size;
    int32_t max_iters;           /* 50 */
    double rel_tol;              /* 1e-3 */
    int32_t estimate_px, estimate_rot, estimate_trans;   /* 1, 1, 1 */
} aar_smooth_fit_params;
typedef struct aar_smooth_fit_report {
    uint32_t struct_size;
    int32_t iterations;          /* EM iterations made */
    int32_t stop_code;           /* 1 = converged, 2 = max_iters */
    double sigma_px, sigma_rot, sigma_trans;       /* physical */
    double sigma_rot_eff, sigma_trans_eff;         /* = physical / sigma_px: the values for aar_smooth_params and aar_tracker_params */
    double last_rel_change;
    int32_t lm_steps;            /* LM iterations of all smoothing runs, the final one included */
    int32_t launches;
    double seconds;
    double a_rot, u_rot, a_trans, u_trans, u_data, data_cost;   /* the last iteration's A_r, U_r, A_t, U_t, U_d and data cost */
} aar_smooth_fit_report;
void aar_smooth_fit_default_params(aar_smooth_fit_params *);   /* struct_size set */
/* Host function (no device needed): AAR_OK or AAR_ERR_INVALID with a message naming the field.  A struct_size that ends before a field leaves
 * it at its default. */
int aar_smooth_fit_params_validate(const aar_smooth_fit_params *);
int aar_track_smooth_fit(aar_problem *, double *x_full, const aar_lm_params *, const aar_smooth_params *, const aar_smooth_fit_params *,
                         double *path, aar_smooth_fit_report *report);
/* One E-step at x_full and the given (effective) sigmas, without smoothing, for checking: pair_terms [num_frames-1][4] = a_r, u_r, a_t, u_t
 * (may be NULL), sums = A_r, U_r, A_t, U_t.  x_full is not modified.  Errors as aar_track_smooth_fit. */
int aar_track_smooth_fit_terms(aar_problem *, const double *x_full, const aar_smooth_params *, double *pair_terms, double sums[4]);
/* The fit for either model.  AAR_SMOOTH_MODEL_RANDOM_WALK: aar_track_smooth_fit / aar_track_smooth_fit_terms themselves,
 * the same bits, sums[4] = sums[5] = 0.  AAR_SMOOTH_MODEL_CONSTANT_VELOCITY: the unknowns are sigma_px and the sigma_rot, sigma_trans of the
 * second-difference terms 1 <= f <= num_frames - 2 (the size of an acceleration per sqrt(unit of frame_time)).  Pair 0's sigma_rot0 and
 * sigma_trans0 are NOT estimated (one pair gives three samples each): they are held at the caller's values as PHYSICAL sigmas, so every
 * smoothing runs at sigma_rot0 / sigma_px, sigma_trans0 / sigma_px next to the effective sigma_rot / sigma_px, sigma_trans / sigma_px.
 * One iteration: aar_track_smooth from the previous track, H at mu = 0, its reduction and the blocks of aar_track_smooth_covariance2, all kept on
 * the device; per term f over the frames p = f-1, c = f, n = f+1, with phi, e_t and the Jacobian rows M_p, M_c, M_n (rotation) and
 * c = (r_f, -(1 + r_f), 1) (translation) of the term at the track, S_xy the blocks of H^-1 between the frames x, y
 *   a_r = |phi|^2 / D_f,  u_r = sum_{x,y} tr(M_x S_xy^ww M_y^T) / D_f,   a_t = |e_t|^2 / D_f,  u_t = sum_{x,y} c_x c_y tr(S_xy^tt) / D_f
 * summed over the terms 1 .. num_frames - 2 ONLY to A_r, U_r, A_t, U_t in a fixed order; entry 0 of the term array is pair 0 in the form of
 * aar_track_smooth_fit, its share of the trace u_0 = u_r[0] / sigma_rot0_eff^2 + u_t[0] / sigma_trans0_eff^2;
 *   U_d = 6 num_frames - U_r / sigma_rot_eff^2 - U_t / sigma_trans_eff^2 - u_0, and with q = sigma_px^2
 *   sigma_rot^2 <- (A_r + q U_r) / (3 (num_frames - 2)),  sigma_trans^2 <- (A_t + q U_t) / (3 (num_frames - 2)),
 *   q <- (data_cost + q U_d) / (8 num_obs),               all three from the old q.
 * The loop, the stop rule, the final smoothing, path, the parameters and the report are aar_track_smooth_fit's.  report->sigma_rot_eff and
 * sigma_trans_eff are the values for aar_smooth_params.sigma_rot / sigma_trans; the matching pair-0 values are sigma_rot0 / report->sigma_px
 * and sigma_trans0 / report->sigma_px.  Bit-reproducible from call to call.
 * AAR_ERR_INVALID: num_frames < 3, no detections, the parameter errors of aar_track_smooth_fit.  AAR_ERR_UNSUPPORTED: with_huber, a
 * communicator.  AAR_ERR_NUMERIC: a non-positive pivot (with the root rule of aar_track_smooth_covariance2), an M-step that gives a variance
 * that is not positive and finite.  On an error nothing is written: x_full, path and report keep their contents. */
int aar_track_smooth_fit2(aar_problem *, double *x_full, const aar_lm_params *, const aar_smooth_params *, const aar_smooth_fit_params *,
                          double *path, aar_smooth_fit_report *report);
/* One E-step at x_full and the given (effective) sigmas, without smoothing, for checking: pair_terms [num_frames-1][4] = a_r, u_r, a_t, u_t,
 * entry 0 = pair 0 (may be NULL), sums = A_r, U_r, A_t, U_t over the terms 1 .. num_frames - 2, u_0, pair 0's cost e_0^T L_0 e_0.  x_full is
 * not modified.  Errors as aar_track_smooth_fit2. */
int aar_track_smooth_fit_terms2(aar_problem *, const double *x_full, const aar_smooth_params *, double *pair_terms, double sums[6]);
/* The smoothed track at any time: pose and covariance at query times that need not be frame times -- a display's vsync,
 * an IMU sample, a camera that is not genlocked.  The answer at a time t is what the smoother would report for a frame WITHOUT detections
 * inserted at t.  With t_0 < ... < t_{F-1} the frame times (frame_time, or 0, 1, 2, ...), z the frame poses of x_full, S_f, R_f the blocks
 * frame_cov, lag_cov of aar_track_smooth_covariance and F(z_i, z_j, D) = J^T L J the 12x12 information of one between factor over D:
 *   inside a gap, t_a < t < t_b (b = a + 1), alpha = (t - t_a) / (t_b - t_a):
 *     pose  R_m = R_a Exp(alpha log(R_a^T R_b)), t_m = t_a + alpha (t_b - t_a), returned as (canonical rvec, t)
 *     cov   the (m, m) block of the inverse of the 18x18 information over (a, b, m):  [S_a R_a; R_a^T S_b]^-1 - F(z_a, z_b, t_b - t_a) on
 *           (a, b), F(z_a, z_m, t - t_a) on (a, m), F(z_m, z_b, t_b - t) on (m, b)
 *   on a frame time, t == t_f exactly: z_f and S_f, bit for bit
 *   outside, t < t_0 or t > t_{F-1} (also num_frames = 1): the pose of the end frame e; cov = the (m, m) block of the inverse of
 *           [S_e^-1 0; 0 0] + F(., ., |t - t_e|), the factor in the order (m, e) before the start and (e, m) after the end
 * query_time [n_query] in any order, duplicates allowed.  pose [n_query][6]; cov [n_query][36] row-major over (rvec, t), symmetric to the bit,
 * UNSCALED (multiply by report->sigma2: an inserted frame adds six residuals and six unknowns, sigma2 is that of the problem as given);
 * segment [n_query] = a inside a gap or on frame a, -1 before the start, num_frames - 1 after the end.  Each of the three and the report may
 * be NULL.  cov = NULL skips the covariance chain: one launch, poses and segments only, and data_cost, prior_cost and sigma2 read 0.
 * All on the device: the chain of aar_track_smooth_covariance, whose blocks stay there, and one thread per query on top.  A query's bits do
 * not depend on the other queries of the call or on their order; two calls give the same bits.  x_full is not modified, no LM state is left.
 * n_query = 0: AAR_OK, nothing written.  Problems created with_huber are accepted (the data blocks carry the weights).
 * AAR_ERR_INVALID (naming the index): a query_time that is not finite, num_frames < 1 with n_query > 0, whatever aar_smooth_params_validate
 * refuses.  AAR_ERR_UNSUPPORTED: rel_motion != NULL -- under an expected motion dR the inserted frame's minimiser has no closed form, because
 * the two parts dR would have to be split into do not commute with the geodesic's steps -- and a problem with a communicator.
 * AAR_ERR_NUMERIC, nothing written: a non-positive pivot in the elimination (as aar_track_smooth_covariance, its root tolerance included) or
 * in any query's own 6x6 inverses. */
typedef struct aar_smooth_query_report {
    uint32_t struct_size;
    int64_t num_residuals, num_vars;   /* of the problem as given, as aar_smooth_covariance_report */
    double data_cost, prior_cost, sigma2;
    int32_t num_queries, num_inside, num_on_frame, num_outside;
    int32_t launches;
    double seconds;
} aar_smooth_query_report;
/* Host function (no device needed): AAR_OK or AAR_ERR_INVALID with a message naming what aar_track_smooth_query would refuse as invalid. */
int aar_smooth_query_validate(int32_t num_frames, const aar_smooth_params *, int64_t n_query, const double *query_time);
int aar_track_smooth_query(aar_problem *, const double *x_full, const aar_smooth_params *, int64_t n_query, const double *query_time,
                           double *pose, double *cov, int32_t *segment, aar_smooth_query_report *report);
/* The same for either model.  AAR_SMOOTH_MODEL_RANDOM_WALK: aar_track_smooth_query itself, the same bits.
 * AAR_SMOOTH_MODEL_CONSTANT_VELOCITY: the second-difference prior is not consistent under subdivision -- inserting a frame replaces up to two
 * terms by up to three and the neighbours move -- so the answer at a time t is what ONE GAUSS-NEWTON STEP of the constant-velocity smoother
 * reports for a frame m without detections inserted at t, linearised at x_full with m at a start pose z_m^0.  With H' the system of the
 * augmented problem at mu = 0 at that point (aar_track_smooth_system2 on the augmented data set: pair 0 on its first two frames, a term on
 * every inner frame with the ratio and L of its own times), g' its right-hand side and g the original one with zero at m:
 *   cov  = (H'^-1)_mm, UNSCALED (report->sigma2 is that of the problem as given)
 *   pose = z_m^0 + delta_m,  delta_m = [H'^-1 (g' - g)]_m, added as aar_track_smooth's trial point adds a step.  g' - g is the contribution
 *          of the changed terms alone, on at most five frames: how far x_full is from converged does not enter.
 * Translations are linear in the model, so delta_m is exactly m's component of the augmented minimiser; for rotations the error is of second
 * order in the step.  The corrections of the other frames are not reported.  Start pose and changed terms:
 *   inside a gap t_a < t < t_b (b = a + 1): z_m^0 the geodesic pose of aar_track_smooth_query; removed: term a (if a >= 1), term b (if
 *     b <= num_frames - 2), pair 0 (if a = 0); added: the term on (a, m, b), on (a - 1, a, m), on (m, b, b + 1), pair 0 on (0, m) likewise
 *   after the end (num_frames >= 2): R_m = R_e Exp(r log(R_{e-1}^T R_e)), t_m = t_e + r (t_e - t_{e-1}), e the last frame, r = (t - t_e) /
 *     D_{e-1}; added: the term on (e - 1, e, m), zero at the start pose -- the pose is the constant-velocity extrapolation to rounding
 *   before the start (num_frames >= 2): R_m = R_0 Exp(-r log(R_0^T R_1)), t_m = t_0 - r (t_1 - t_0), r = (t_0 - t) / D_0; removed: pair 0;
 *     added: pair 0 on (m, 0) and the term on (m, 0, 1)
 *   num_frames = 1, outside: aar_track_smooth_query's formula with sigma_rot0, sigma_trans0; the pose is z_0
 *   on a frame time: z_f and frame_cov[f] of aar_track_smooth_covariance2, bit for bit
 * Arguments, segment, the three counts and the report are aar_track_smooth_query's.  All on the device: the chain of
 * aar_track_smooth_covariance2, whose blocks stay there, the lag-three blocks (H^-1)_{f,f+3}, and one wavefront per query.  cov = NULL still
 * runs the whole chain -- the pose depends on the block -- and saves the copy back alone.  A query's bits depend on its time and the track
 * alone; two calls give the same bits; blocks symmetric to the bit.  x_full is not modified, no LM state is left.  n_query = 0: AAR_OK, nothing
 * written.  Problems created with_huber are accepted.
 * AAR_ERR_INVALID: whatever aar_smooth_query_validate refuses.  AAR_ERR_UNSUPPORTED: a problem with a communicator.  AAR_ERR_NUMERIC, nothing
 * written: a non-positive pivot in the elimination (with the root rule of aar_track_smooth_covariance2), in a supernode block of the lag-three
 * blocks or in a query's own eliminations. */
int aar_track_smooth_query2(aar_problem *, const double *x_full, const aar_smooth_params *, int64_t n_query, const double *query_time,
                            double *pose, double *cov, int32_t *segment, aar_smooth_query_report *report);
/* For checking, constant velocity only (the random walk is AAR_ERR_UNSUPPORTED): the two summands of aar_track_smooth_query2's pose on their
 * own, start_pose [n_query][6] = z_m^0 and step [n_query][6] = delta_m (pose = start_pose + step to the bit; on a frame time z_f and zero).
 * The sum rounds delta_m to eps |z_m|, so a step can only be held to its own accuracy from here.  Either may be NULL; errors as above. */
int aar_track_smooth_query2_step(aar_problem *, const double *x_full, const aar_smooth_params *, int64_t n_query, const double *query_time,
                                 double *start_pose, double *step);
/* For checking, constant velocity only (the random walk is AAR_ERR_UNSUPPORTED): lag3_cov [num_frames-3][36] = (H^-1)_{f,f+3}, row-major, the
 * rows belong to frame f, UNSCALED -- the blocks aar_track_smooth_query2 takes beside those of aar_track_smooth_covariance2.  On supernodes
 * (2k, 2k + 1) an even f is a block of the selected inverse; an odd f = 2k - 1 follows from the Gauss-Markov property of the block-tridiagonal
 * chain, Sigma_{k-1,k+1} = Sigma_{k-1,k} Sigma_kk^-1 Sigma_{k,k+1}.  num_frames < 4: AAR_OK, nothing written.  Errors as above. */
int aar_track_smooth_lag3(aar_problem *, const double *x_full, const aar_smooth_params *, double *lag3_cov);
/* The covariance between ANY two frames of the smoothed track and the relative motion between them: how far did the
 * object move and turn between frame a and frame b, and how sure is that?  Either model (aar_smooth_params.model).  H is the system
 * aar_track_smooth_system2 returns at mu = 0 for the same x_full and parameters, Sigma = H^-1; everything is UNSCALED (multiply by
 * report->sigma2), as everywhere else.  Per pair q = (a, b) = (frame_a[q], frame_b[q]), in any order, a > b and duplicates allowed:
 *   cross_cov[q] = Sigma_ab, row-major, the rows belong to frame a.  (b, a) is the transpose of (a, b) to the bit.  a = b: frame_cov[a];
 *                  |a - b| = 1: lag_cov; under constant velocity |a - b| = 2: lag2_cov, |a - b| = 3: the blocks of aar_track_smooth_lag3 --
 *                  the bits those calls return.  Beyond that the Gauss-Markov chain of a block-tridiagonal H (in frames under the random walk,
 *                  in supernodes (2k, 2k + 1) under constant velocity): Sigma_ab = Sigma_ak Sigma_kk^-1 Sigma_kb for a < k < b, one 6x6 (12x12)
 *                  product per step of the lag, no new solve.
 *   rel[q]       = [log(R_a^T R_b)^v ; t_b - t_a]: the smoother's own between without an expected motion (also when rel_motion is set, which
 *                  changes H alone) -- the rotation in frame a's body frame, the translation in the root camera's frame.
 *   rel_cov[q]   = J_a Sigma_aa J_a^T + J_b Sigma_bb J_b^T + J_a Sigma_ab J_b^T + (J_a Sigma_ab J_b^T)^T, J_a = [M_a 0; 0 -I], J_b = [M_b 0; 0 I]
 *                  the between's Jacobians; symmetric to the bit.  With smoothing sigmas tight enough to pay off, nearby frames share most of
 *                  their error: Sigma_aa + Sigma_bb overstates this by a large factor and only Sigma_ab corrects it.
 *                  a = b: zeros exactly, in rel and rel_cov.
 * A velocity over the baseline is rel / (t_b - t_a) with covariance rel_cov / (t_b - t_a)^2.
 * Each of the three outputs and the report may be NULL.  x_full is not modified and no LM state is left behind.  n_pairs = 0: AAR_OK, no
 * output written (the report holds the counts alone).  Problems created with Huber are accepted.  A query's bits depend on (a, b) and the
 * track alone, not on the other queries or their order; two calls give the same bits.  The cost of a query is O(|a - b|).
 * AAR_ERR_INVALID (naming the index): an index outside [0, num_frames), null arrays with n_pairs > 0, whatever aar_smooth_params_validate
 * refuses.  AAR_ERR_UNSUPPORTED: a problem with a communicator.  AAR_ERR_NUMERIC, nothing written: a non-positive pivot in the elimination (with
 * the root rules of aar_track_smooth_covariance / aar_track_smooth_covariance2), in a supernode block of the lag-three blocks, or in a Sigma_kk
 * that the chain inverts. */
typedef struct aar_smooth_relative_report {
    uint32_t struct_size;
    int64_t num_residuals, num_vars;   /* of the problem as given, as aar_smooth_covariance_report */
    double data_cost, prior_cost, sigma2;
    int32_t num_pairs, num_direct, num_chained, max_lag;   /* direct: answered from the blocks that exist (lag <= 1; <= 3 under constant velocity) */
    int32_t launches;
    double seconds;
} aar_smooth_relative_report;
/* Host function (no device needed): AAR_OK or AAR_ERR_INVALID with a message naming what aar_track_smooth_relative would refuse as invalid. */
int aar_smooth_relative_validate(int32_t num_frames, const aar_smooth_params *, int64_t n_pairs, const int32_t *frame_a, const int32_t *frame_b);
int aar_track_smooth_relative(aar_problem *, const double *x_full, const aar_smooth_params *, int64_t n_pairs, const int32_t *frame_a,
                              const int32_t *frame_b, double *cross_cov, double *rel, double *rel_cov, aar_smooth_relative_report *report);
/* Per-detection diagnostics of a SMOOTHED track: what aar_problem_predict_corners, _detection_leverage,
 * _detection_loo and _gate_detections are to the bundle, with the smoother's own covariance.  Either model.  With z_f the frame poses of
 * x_full, H the system aar_track_smooth_system2 returns at mu = 0 for the same arguments (the cameras and markers are constants, the motion
 * prior is in), Sigma = H^-1 UNSCALED, cost = data_cost + prior_cost, nu = num_residuals - num_vars = 8 N - 6 and sigma2 = cost / nu as
 * aar_smooth_covariance_report has them: for a detection i of frame f, u_i its four projected corners, G_i = du_i / dz_f (8 x 6, the
 * smoother's own frame Jacobian, without the Huber weights) and C_i = G_i Sigma_ff G_i^T (8 x 8, symmetric to the bit).
 * aar_track_smooth_detection_leverage, the problem's detections in reference order:
 *   leverage[i] = tr(C_i), row_leverage[i][k] = C_i[k][k].  Without Huber  sum_i leverage_i = 6 F - tr(Sigma H_prior),  H_prior = H minus the
 *   frames' data blocks (a frame without detections contributes nothing to the sum): what the prior determines is not the detections' to
 *   determine.  With Huber the call is allowed and the identity is not claimed: Sigma carries the weights and G does not, as in the bundle.
 * aar_track_smooth_detection_loo: the quantities of aar_problem_detection_loo with this C_i, this cost and this nu --
 *   r_i = observed - u_i, loo_resid = (I - C_i)^-1 r_i, q = r_i^T (I - C_i)^-1 r_i, F = (q / 8) / ((cost - q) / (nu - 8)) (+inf where the
 *   denominator is <= 0, NaN where nu <= 8), cook = w^T C_i w / (6 F sigma2), margin = the smallest pivot met, keep = 0 iff a rule is
 *   given, status == 0 and F > f_max.  status bit 0 (AAR_PREDICT_BEHIND): outputs NaN, keep = 1.  Bit 2 (AAR_PREDICT_UNDETERMINED): a pivot
 *   of I - C_i is <= 1e-6 or not finite; leverage and margin are written, the rest is NaN, keep = 1 -- the detection alone carries some
 *   direction of its frame's pose: its frame has no other detection and no neighbour reaches it through the prior (one frame with one
 *   detection).  Bit 1 is never set: a smoothed track whose chain succeeded has a block for every frame.  Every array may be NULL.
 *   A problem created with_huber is AAR_ERR_UNSUPPORTED (the weights break the Gaussian data model the statistic rests on); a rule whose
 *   f_max is not positive and finite is AAR_ERR_INVALID.
 * aar_track_smooth_predict_corners: for any camera index, marker index and TIME the four corners at the pose aar_track_smooth_query2
 *   reports for that time and C = G Sigma_t G^T with Sigma_t that query's 6 x 6 block.  sigma2 C is the corners' covariance and
 *   sigma2 (C + I) the search window of a new detection at that time: the next frame, a camera that is not genlocked, a vsync.  At
 *   (cam_i, marker_i, frame_time[f_i]) of the problem's own detections the diagonal of cov is row_leverage to the bit.  cov == NULL under
 *   the random walk runs no selected inverse.  Duplicates are allowed; a query's bits depend on its triple and the track only.  Camera and
 *   marker indices are checked as aar_predict_query_validate checks them, times as aar_smooth_query_validate; rel_motion != NULL is
 *   AAR_ERR_UNSUPPORTED as in aar_track_smooth_query.  status bit 0: uv and cov NaN.
 * aar_track_smooth_gate_detections: the same queries with observed corners uv_obs; innovation = uv_obs - u, m2 = e^T (I + C)^-1 e,
 *   UNSCALED (m2 / sigma2 is chi-square with 8 degrees of freedom under the model); status as above.
 * All four validate as every smoother entry does, are AAR_ERR_UNSUPPORTED behind a communicator, leave no LM state, do not modify x_full
 * and write the caller's arrays only after everything succeeded; a non-positive pivot of the chain is AAR_ERR_NUMERIC with the chain's
 * own message.  Two calls give the same bits.  The reports are size-versioned: the caller sets struct_size, at most that many bytes are
 * filled; they may be NULL. */
typedef struct aar_smooth_predict_report {
    uint32_t struct_size;
    int64_t num_residuals, num_vars;   /* of the problem as given, as aar_smooth_covariance_report */
    double data_cost, prior_cost, sigma2;   /* 0 where no selected inverse ran */
    int64_t num_queries, behind;       /* queries (the problem's detections for detection_leverage), those with status bit 0 */
    double leverage_sum;               /* sum of the finite tr(C) in query order (gate_detections: 0) */
    int32_t num_inside, num_on_frame, num_outside;   /* time queries, as aar_smooth_query_report */
    int32_t launches;
    double seconds;
    double kernel_seconds;             /* the query kernel's own time between two events; 0 unless aar_set_kernel_profiling is on */
} aar_smooth_predict_report;
typedef struct aar_smooth_loo_report {
    uint32_t struct_size;
    int64_t num_residuals, num_vars;
    double data_cost, prior_cost, sigma2;
    int64_t dof;                       /* nu = num_residuals - num_vars */
    int64_t behind, undetermined, rejected;   /* detections with status bit 0 / bit 2 / keep = 0 */
    double f_max, max_f;               /* the rule's (+inf without one); the largest F that is not NaN (NaN when there is none) ... */
    int64_t argmax_f;                  /* ... and its detection (-1) */
    double leverage_sum;               /* sum of the finite leverages in detection order */
    int32_t launches;
    double seconds;
    double kernel_seconds;             /* as aar_smooth_predict_report */
} aar_smooth_loo_report;
int aar_track_smooth_detection_leverage(aar_problem *, const double *x_full, const aar_smooth_params *, double *leverage /* [N] */,
                                        double *row_leverage /* [N][8], may be NULL */, aar_smooth_predict_report *report);
int aar_track_smooth_detection_loo(aar_problem *, const double *x_full, const aar_smooth_params *, const aar_loo_rule *rule /* may be NULL */,
                                   double *loo_resid /* [N][8] */, double *q, double *F, double *cook, double *leverage, double *margin /* [N] */,
                                   uint8_t *status, uint8_t *keep /* [N] */, aar_smooth_loo_report *report);
int aar_track_smooth_predict_corners(aar_problem *, const double *x_full, const aar_smooth_params *, int64_t n_query, const int32_t *q_cam,
                                     const int32_t *q_marker, const double *q_time, double *uv /* [n][8] */, double *cov /* [n][64] or NULL */,
                                     uint8_t *status, int32_t *segment /* [n] or NULL, as aar_track_smooth_query */,
                                     aar_smooth_predict_report *report);
int aar_track_smooth_gate_detections(aar_problem *, const double *x_full, const aar_smooth_params *, int64_t n_query, const int32_t *q_cam,
                                     const int32_t *q_marker, const double *q_time, const float *uv_obs /* [n][8] */,
                                     double *innovation /* [n][8] */, double *m2 /* [n] */, uint8_t *status, int32_t *segment,
                                     aar_smooth_predict_report *report);
/* YAML (the dialect of aar_loo_write_yaml) of a smoothed track's leave-one-out report, of a single-GPU problem created from d: the report's
 * scalars (sigma2, data_cost, prior_cost, dof, f_max, max_f, undetermined, rejected, leverage_sum); per camera id and marker id
 * {detections, max_f, rejected}; the detections with keep = 0 or an UNDETERMINED status as (frame id, camera id, marker id, F, q, leverage,
 * error).  F, status and keep are required when d has detections; q, leverage and det_err may be NULL (.nan).  Host code. */
int aar_smooth_loo_write_yaml(const char *path, const aar_dataset *d, const double *F, const double *q, const double *leverage,
                              const double *det_err, const uint8_t *status, const uint8_t *keep, const aar_smooth_loo_report *report);

/* Live tracker (no counterpart in the reference as one object: it is the body of apps/track.cpp's loop, :102-136, kept on the device; DESIGN.md
 * section 17).  Created from a solution -- cameras, markers, cam_mats, marker_size and the roots; the solution's own frames and detections are
 * ignored -- and then fed ONE FRAME PER CALL, in time order.  After push n the window holds the last W = min(n + 1, lag + 1) pushed frames: these
 * are still refined.  The frame that has just left the window (n - lag - 1, if it exists) is the anchor: its pose is final and held fixed.
 *   smooth = 0 (needs lag = 0): no prior.  A push minimises E_n(z_n) exactly as aar_track does for one frame (rows = 8 n_obs); a frame without
 *     detections keeps its start, with 0 iterations.
 *   smooth = 1: a push minimises over the window's poses
 *         E = sum_{f in window} E_f(z_f) + sum_{f, f+1 in window} e_f^T L_f e_f + [anchor exists] e_a^T L_a e_a
 *     with e_f, L_f as in aar_track_smooth (D_f from the pushes' frame_time, no rel_motion) and e_a = e(z_anchor, z_first), z_anchor constant.
 *     The LM is aar_track_smooth's, restarted on every push: mu = tau max diag H over the window's blocks, v = 2, the gain test with at most five
 *     retries, exits 1 / 2 / 3 with rows = 8 (detections in the window) + 6 (pairs, the anchor pair included); a non-positive pivot of the
 *     block-tridiagonal solve rejects the try.  Frames without detections are allowed: the prior carries them.
 *   The new frame starts from pose_init when given, otherwise from the current estimate of the previous frame (the first push must give one);
 *   older window frames start from their estimates after the previous push.  E_f uses double residuals and, with with_huber, Huber weights
 *   with huber_delta; the prior is never Huber-weighted.
 * One push is one host -> device copy of the frame's records, ONE kernel launch (the whole LM runs inside it) and one device -> host copy of the
 * result.  Two trackers fed the same pushes give the same bits.  A rejected push (AAR_ERR_INVALID, the message names the entry) leaves the
 * tracker exactly as it was.  Structs are size-versioned: the caller sets struct_size. */
#define AAR_TRACKER_MAX_LAG 15
#define AAR_TRACKER_ANCHOR_FIXED 0      /* the frame that leaves the window becomes a constant (above) */
#define AAR_TRACKER_ANCHOR_MARGINAL 1   /* ... is marginalised into a 6x6 Gaussian prior on the frame behind it (below) */
typedef struct aar_tracker aar_tracker;
typedef struct aar_tracker_params {
    uint32_t struct_size;
    int32_t lag;                 /* 0 .. AAR_TRACKER_MAX_LAG: frames that stay in the window behind the newest one */
    int32_t smooth;              /* 0 | 1; 0 requires lag = 0 */
    double sigma_rot;            /* rad   per sqrt(unit of frame_time), > 0 finite when smooth */
    double sigma_trans;          /* metre per sqrt(unit of frame_time), > 0 finite when smooth */
    int32_t with_huber;          /* 0 | 1 */
    float huber_delta;           /* pixels, > 0 finite when with_huber */
    int32_t max_obs_per_frame;   /* >= 1: detections one push may carry (sizes the ring) */
    int32_t device_id;
    int32_t anchor_mode;         /* AAR_TRACKER_ANCHOR_FIXED (default) | AAR_TRACKER_ANCHOR_MARGINAL (needs smooth = 1 and lag >= 1) */
    int32_t covariance;          /* 0 | 1: every push also leaves the window's pose covariance blocks for aar_tracker_uncertainty */
} aar_tracker_params;
typedef struct aar_tracker_result {
    uint32_t struct_size;
    int64_t frame_index;         /* n: pushes accepted before this one */
    int32_t window_frames;       /* W */
    int32_t iterations, stop_code, rejected_tries;
    double initial_cost, final_cost, final_data_cost, final_prior_cost, final_mu;
    double pose[6];              /* the newest frame */
    int32_t has_lagged;          /* the window is full: lagged_pose is the oldest window frame, which becomes the anchor at the next push --
                                    its final, fixed-lag smoothed value */
    int64_t lagged_index;
    double lagged_pose[6];
    double seconds;              /* wall time of the push */
} aar_tracker_result;
void aar_tracker_default_params(aar_tracker_params *);   /* struct_size set; lag 0, smooth 0, no Huber (delta 2.5), 256 detections, device 0 */
/* Host function (no device needed): AAR_OK or AAR_ERR_INVALID with a message naming the field: lag out of range, smooth = 0 with lag > 0, a
 * sigma that is not positive and finite when smooth is set, huber_delta likewise when with_huber is set, max_obs_per_frame < 1, a malformed
 * solution (sizes, roots, null arrays, a non-finite camera / marker pose or marker_size), an unknown anchor_mode, AAR_TRACKER_ANCHOR_MARGINAL
 * with smooth = 0 or lag = 0, covariance not 0 / 1.  A struct_size that ends before anchor_mode means fixed anchor, no covariance. */
int aar_tracker_params_validate(const aar_dataset *solution, const aar_tracker_params *);
int aar_tracker_create(const aar_dataset *solution, const aar_tracker_params *, const aar_lm_params * /* NULL = defaults */, aar_tracker **out);
/* obs_cam / obs_marker: INDICES into the solution's cameras / markers, obs_uv: [n_obs][8] undistorted corners, pose_init: [6] (rvec, t) or NULL.
 * Rejected (AAR_ERR_INVALID): n_obs above max_obs_per_frame, an index out of range, a frame_time that is not finite or not above the previous
 * one, a missing first pose_init, a non-finite pose_init.  result may be NULL. */
int aar_tracker_push(aar_tracker *, double frame_time, int32_t n_obs, const int32_t *obs_cam, const int32_t *obs_marker, const float *obs_uv,
                     const double *pose_init, aar_tracker_result *result);
/* The current window, oldest frame first (to flush the end of a stream): n = W, frame_index [n], poses [n][6], frame_err [n] = E_f, pair_err [n] =
 * cost of the pair that ENDS at the frame (entry 0: the anchor pair, 0 without an anchor), anchor_pose, has_anchor.  Any output may be NULL. */
int aar_tracker_window(aar_tracker *, int32_t *n, int64_t *frame_index, double *poses, double *frame_err, double *pair_err, double anchor_pose[6],
                       int32_t *has_anchor);
int aar_tracker_reset(aar_tracker *);     /* forgets all frames, the marginal prior (and aar_tracker_enable_detections / _enable_gate / _enable_motion), keeps the solution */

/* Marginalised anchor and per-push pose covariance.  Both are off by default, and then a push runs the same kernel and
 * gives the same bits as before they existed; with either set a push is still one launch and one copy back.
 *   anchor_mode = AAR_TRACKER_ANCHOR_MARGINAL (smooth = 1, lag >= 1; lag = 0 is refused and left for later: the next pair's time step is not
 *     known when the frame leaves).  The anchor pair is replaced by a prior on the first window frame, E_m(z_0) = (z_0 - m)^T L_m (z_0 - m),
 *     which counts 6 rows where the anchor pair did.  At the end of every push with a full window the oldest frame is marginalised at the final
 *     point z^: from one fresh system at mu = 0, with A, a the first diagonal block and right-hand side (old prior, E_0 and the J_a half of pair
 *     (0, 1)), O the first off-diagonal block and B, c the J_b half of pair (0, 1) alone,
 *         L' = B - O^T A^-1 O,   b' = c - O^T A^-1 a,   m' = z^_1 + L'^-1 b'
 *     and (L', m') is the prior of the next push.  When L' has a non-positive pivot -- below 1e-10 of the matching diagonal entry of B, which is
 *     how an exact 0 shows in floating point: a leaving frame with neither prior nor detections -- the next push carries no prior and
 *     marginal_dropped counts it.  The fixed anchor_pose of aar_tracker_window is still kept.
 *   covariance = 1 (any anchor_mode, also smooth = 0): from the same fresh system, the diagonal 6x6 blocks of H^-1 (H = J^T J over the window's
 *     6 W unknowns, prior and pairs included) for every window frame, by the block elimination's backward recursion.  They are reported
 *     UNSCALED with sigma2 = final_cost / (rows - 6 W), 0 when rows <= 6 W (the convention of aar_problem_covariance).  A non-positive pivot
 *     (smooth = 0 on a frame without detections) gives cov_valid = 0 and zeros.
 * aar_tracker_uncertainty is served from the host copy of the last accepted push (no device work) and describes the tracker after that push:
 * cov [i] belongs to frame_index [i], oldest first; has_marginal / marginal_index / marginal_info / marginal_mean are the prior the NEXT push
 * will put on frame marginal_index.  AAR_ERR_INVALID before any push, after a reset, with both options off, or after a push that failed with
 * AAR_ERR_HIP (its copy has overwritten the record; a push rejected with AAR_ERR_INVALID leaves it as it was).  out is size-versioned. */
typedef struct aar_tracker_uncertainty_record {
    uint32_t struct_size;
    int32_t cov_valid;
    double sigma2;
    int32_t window_frames;
    int32_t has_marginal;
    int64_t frame_index[AAR_TRACKER_MAX_LAG + 1];
    double cov[AAR_TRACKER_MAX_LAG + 1][36];   /* row-major 6x6 over (rvec, t), zeros past window_frames */
    int64_t marginal_index;      /* -1 without a marginal */
    double marginal_info[36];    /* L_m, row-major */
    double marginal_mean[6];     /* m */
    int64_t marginal_dropped;    /* pushes since creation / reset whose marginal was dropped */
} aar_tracker_uncertainty_record;
int aar_tracker_uncertainty(aar_tracker *, aar_tracker_uncertainty_record *out);
/* The lagged covariance blocks of a live run as YAML, in aar_covariance_write_yaml's dialect: object_poses holds one record per frame of d
 * (frame_id, sigma_rot, sigma_trans, covariance = frame_sigma2[f] * frame_cov[f], a block of NaN where valid[f] is 0), frame_sigma2 one
 * { frame_id, sigma2 } per frame.  frame_cov: [num_frames][36] unscaled, frame_sigma2 / valid: [num_frames]. */
int aar_tracker_covariance_write_yaml(const char *path, const aar_dataset *d, const double *frame_cov, const double *frame_sigma2,
                                      const uint8_t *valid);

/* The live tracker fed RAW detections: the first half of apps/track.cpp's loop (:117-133) on the device as well.  Per push
 * the frame's corners are undistorted with the camera's K and up to AAR_MAX_DIST coefficients (they replace the raw ones in the window, so the
 * refinement sees what aar_tracker_push would be given), IPPE runs on every detection (obtain_pose_estimations), the object pose candidates of
 * init_object_transforms are enumerated in the reference's order -- by marker index, then camera index; first solution, then the second when
 * (double)e2 / (double)e1 < ippe_threshold -- and voted on (find_best_transformation: first minimum of the summed corner distances, NaN never
 * wins; a candidate with a non-finite entry is also left out of the other candidates' sums).  All of it is ONE extra launch of one workgroup
 * (k_live_init) in front of aar_tracker_push's launch: one copy in, two launches, one copy out that carries result and info; nothing is
 * allocated per push.  The start of the new frame:
 *   pose_init given, policy VOTE          no vote: aar_tracker_push on the undistorted corners
 *   n_det < min_detections                no vote: pose_init, else the previous estimate; neither (first push) -> AAR_ERR_INVALID
 *   policy VOTE                           the vote's winner; no finite candidate -> the previous estimate, without one AAR_ERR_NUMERIC
 *   policy BEST                           prediction = pose_init, else the previous estimate.  The new frame's data cost E_f is evaluated at the
 *                                         prediction and at the vote's winner; the vote starts the frame only when strictly cheaper.  Without a
 *                                         prediction the vote alone decides; without a finite candidate the prediction does.
 * Only a first push without pose_init can be rejected after the device has run (the host then waits for k_live_init before it launches the
 * refinement); every rejected push leaves the tracker exactly as it was.  max_obs_per_frame above 4096 is AAR_ERR_UNSUPPORTED here: the vote
 * is quadratic in the candidates (at most two per detection) on one compute unit. */
#define AAR_TRACKER_START_VOTE 1   /* every frame without a pose_init starts from its own vote (the reference's loop) */
#define AAR_TRACKER_START_BEST 2   /* the cheaper of {pose_init or previous estimate, vote} in the new frame's data cost */
typedef struct aar_tracker_detection_params {
    uint32_t struct_size;
    const aar_cam_model *cams;   /* [solution->num_cams] by camera INDEX; NULL = the solution's cam_mats + its 5 dist_coeffs */
    double ippe_threshold;       /* default 2.0 (aar_init_params.threshold) */
    int32_t min_detections;      /* default 2: fewer usable detections -> no vote for that frame */
    int32_t start_policy;        /* default AAR_TRACKER_START_VOTE */
} aar_tracker_detection_params;
typedef struct aar_tracker_start_info {
    uint32_t struct_size;
    int32_t voted;               /* a vote was held */
    int32_t candidates, winner;  /* winner: index in candidate order, -1 = none finite */
    double vote_cost;            /* the winner's summed error (find_best_transformation's weight) */
    int32_t start_source;        /* 0 pose_init, 1 previous estimate, 2 vote, 3 motion prediction (aar_tracker_enable_motion) */
    double cost_prediction, cost_vote;  /* new frame's E_f at the two starts (BEST with both a prediction and a winner, else 0) */
    double start_pose[6];
} aar_tracker_start_info;
void aar_tracker_default_detection_params(aar_tracker_detection_params *);   /* struct_size set; cams NULL, 2.0, 2, AAR_TRACKER_START_VOTE */
/* Host function (no device needed): AAR_OK or AAR_ERR_INVALID with a message naming the field: a struct_size that does not reach start_policy,
 * ippe_threshold not positive and finite, min_detections < 1, an unknown start_policy, a cams entry with a non-finite K / dist or a bad n_dist. */
int aar_tracker_detection_params_validate(const aar_dataset *solution, const aar_tracker_detection_params *);
/* Once after aar_tracker_create or aar_tracker_reset, before the first push; again without a reset: AAR_ERR_INVALID.  The cams array is copied. */
int aar_tracker_enable_detections(aar_tracker *, const aar_tracker_detection_params *);
/* det_cam / det_marker: INDICES into the solution's cameras / markers, det_uv_raw: [n_det][8] corners as detected.  Rejections as
 * aar_tracker_push, plus a call before aar_tracker_enable_detections.  result and info may be NULL.  May be mixed with aar_tracker_push. */
int aar_tracker_push_detections(aar_tracker *, double frame_time, int32_t n_det, const int32_t *det_cam, const int32_t *det_marker,
                                const float *det_uv_raw, const double *pose_init /* may always be NULL */,
                                aar_tracker_result *, aar_tracker_start_info *);
void aar_tracker_destroy(aar_tracker *);

/* Tracker bank: B independent live trackers -- one per object of a rig, each with its own solution, all with the same
 * aar_tracker_params and aar_lm_params -- that advance in lockstep, one frame per call.  Member b is exactly an aar_tracker created from
 * solutions[b]: same window, same LM, same anchor / covariance options, same start rules; nothing couples the members.  On the device member b is
 * workgroup b of ONE launch, so a bank push is ONE host -> device copy (the ring is laid out [slot][member]: the slots a push fills are contiguous),
 * ONE launch of B workgroups (TWO on a push of raw detections) and ONE device -> host copy, whatever B.  All memory is allocated by
 * aar_tracker_bank_create (the detection workspaces by aar_tracker_bank_enable_detections), nothing per push.  Members may differ in their
 * numbers of cameras and markers; max_obs_per_frame bounds every member's n_obs / n_det.
 * A bank push is all or nothing: when any member's input is rejected (AAR_ERR_INVALID, the message names the member and the entry), the time does
 * not ascend, or -- first push of raw detections -- a member has no finite candidate and nothing to fall back on (AAR_ERR_NUMERIC, the message
 * names the member), every member stays exactly as it was. */
#define AAR_TRACKER_BANK_MAX_MEMBERS 1024
typedef struct aar_tracker_bank aar_tracker_bank;
typedef struct aar_tracker_bank_stats {
    uint32_t struct_size;
    int32_t members;
    int64_t pushes;              /* accepted */
    int64_t launches;            /* kernel launches, counted on the host where they are issued (rejected pushes included) */
    int64_t h2d_copies, h2d_bytes;
    int64_t d2h_copies, d2h_bytes;
} aar_tracker_bank_stats;
/* Host function (no device needed): AAR_ERR_INVALID for n_members outside 1 .. AAR_TRACKER_BANK_MAX_MEMBERS, a null entry of solutions, or a
 * member that aar_tracker_params_validate refuses (the message then starts with "member b: "). */
int aar_tracker_bank_params_validate(int32_t n_members, const aar_dataset *const *solutions, const aar_tracker_params *);
int aar_tracker_bank_create(int32_t n_members, const aar_dataset *const *solutions, const aar_tracker_params *,
                            const aar_lm_params * /* NULL = defaults */, aar_tracker_bank **out);
int32_t aar_tracker_bank_size(const aar_tracker_bank *);   /* B; 0 for NULL */
/* n_obs: [B]; obs_cam / obs_marker / obs_uv: the members' frames one behind the other (member 0's n_obs[0] detections first), indices into the
 * MEMBER's solution.  n_obs[b] = 0: object b was not seen -- the frame is bridged by the prior (smooth = 1) or keeps its start (smooth = 0), as
 * in aar_tracker_push.  pose_init: [B][6] or NULL; has_init: [B], nonzero = member b's row of pose_init is given, NULL = every row is (when
 * pose_init is not NULL).  The first push needs a start for every member.  results: [B] (every struct_size set) or NULL. */
int aar_tracker_bank_push(aar_tracker_bank *, double frame_time, const int32_t *n_obs, const int32_t *obs_cam, const int32_t *obs_marker,
                          const float *obs_uv, const double *pose_init, const uint8_t *has_init, aar_tracker_result *results);
/* per_member: [B] or NULL, a NULL entry (or NULL array) = aar_tracker_default_detection_params for that member.  As
 * aar_tracker_enable_detections: once after create or reset, before the first push. */
int aar_tracker_bank_enable_detections(aar_tracker_bank *, const aar_tracker_detection_params *const *per_member);
/* aar_tracker_push_detections for every member (n_det: [B], the arrays concatenated as above); infos: [B] or NULL.  On a first push in which
 * some member has no pose_init the host waits for the start kernel before it launches the refinement, as the single tracker does. */
int aar_tracker_bank_push_detections(aar_tracker_bank *, double frame_time, const int32_t *n_det, const int32_t *det_cam, const int32_t *det_marker,
                                     const float *det_uv_raw, const double *pose_init, const uint8_t *has_init, aar_tracker_result *results,
                                     aar_tracker_start_info *infos);
/* aar_tracker_window / aar_tracker_uncertainty of one member */
int aar_tracker_bank_window(aar_tracker_bank *, int32_t member, int32_t *n, int64_t *frame_index, double *poses, double *frame_err, double *pair_err,
                            double anchor_pose[6], int32_t *has_anchor);
int aar_tracker_bank_uncertainty(aar_tracker_bank *, int32_t member, aar_tracker_uncertainty_record *out);
int aar_tracker_bank_reset(aar_tracker_bank *);   /* aar_tracker_reset for every member; the counters of aar_tracker_bank_get_stats stay */
/* out->struct_size: the caller's sizeof; at most that many bytes are written and struct_size says how many were. */
int aar_tracker_bank_get_stats(const aar_tracker_bank *, aar_tracker_bank_stats *out);
void aar_tracker_bank_destroy(aar_tracker_bank *);

/* per-stage device time of the last aar_lm_solve, seconds, in the reference's verbose-timer vocabulary
 * (libs/sparselevmarq.h:425) extended with the stages that only exist here */
typedef struct aar_stage_times {
    double unpack, jacobian_normal_eq, schur, chol, backsub, residual, control, allreduce, total;
    int64_t launches;
} aar_stage_times;
int aar_get_stage_times(aar_problem *, aar_stage_times *);
/* Stage timers on / off (also on with AAR_STAGE_TIMERS=1 in the environment when the problem is created): every stage of a
 * step is then bracketed by two HIP events on the library's stream and waited for, which serialises host and device -- a
 * diagnostic mode (bench.py's `amdahl` object, the verbose stage line), not the production path.  Resets the accumulators. */
int aar_set_stage_timers(aar_problem *, int on);

/* out[0] = CG iterations of the last damped solve, out[1] = their running total since the problem was created (zeros for AAR_SOLVER_DIRECT);
 * aar_problem_get_solver_stats says more */
int aar_problem_pcg_iterations(aar_problem *, int32_t out[2]);

/* Per-kernel device time: when profiling is on, every kernel launch of this problem is bracketed by two HIP
 * events on the library's own stream (the stream the kernels run on) and the elapsed times are accumulated
 * per kernel.  bench.py's roofline figures come from here.  Switching profiling on resets the accumulators. */
#define AAR_NUM_KERNELS 18
int aar_set_kernel_profiling(aar_problem *, int on);
int aar_get_kernel_times(aar_problem *, double seconds[AAR_NUM_KERNELS], int64_t launches[AAR_NUM_KERNELS]);
const char *aar_kernel_name(int kernel_id);

/* fp64 reprojection statistics at x_full (device): per-corner RMSE sqrt(sum r^2 / 4N), sum r^2 */
int aar_reproj_stats(aar_problem *, const double *x_full, double *rmse, double *sum_sq);

int aar_device_count(void);
int aar_device_synchronize(void);

/* The gate of the live trackers: aar_outlier_rule of the residual report above, applied on the device to the NEW frame of
 * every push, as ONE extra launch between the frame's start and its refinement.  Definitions, word for word those of the residual report:
 *   start pose  z0 = the pose the push starts from: the caller's pose_init, else what the start kernel wrote (the vote's winner, or the choice of
 *               AAR_TRACKER_START_BEST), else the previous frame's current estimate
 *   e_d         sqrt((sum over the 4 corners of rx^2 + ry^2) / 4) in pixels at z0: fp64, summed in corner order, UNWEIGHTED (Huber is ignored),
 *               the tracker's double residuals
 *   median      the exact lower median (element floor((n-1)/2) of the ascending order), max the exact maximum; a non-finite e_d sorts above
 *               every finite one (and reads as +inf in median / max)
 *   threshold   t = max(min_px, k_median * median) in fp64; k_median <= 0: t = min_px
 *   kept        iff e_d <= t, so a non-finite e_d never is
 * A frame of fewer than min_detections detections is not gated: everything is kept, gated = 0, threshold = +inf.  The kept detections stay in
 * the caller's order; the refinement, aar_tracker_result.final_data_cost, the window's frame_err and the rows all see the kept detections only,
 * with the bits an ungated tracker gives when the caller leaves the rejected detections out.  A gate that keeps nothing is legal: the frame
 * then is a push with n_obs = 0.  AAR_TRACKER_START_BEST evaluates its two starts on ALL detections: the start kernel runs before the gate.
 * A gated push is the ungated push's launches plus one; still one copy in and one copy out, and no host wait in between (except, as before,
 * on a first raw push without pose_init).  max_obs_per_frame above 4096 with the gate is AAR_ERR_UNSUPPORTED (the median sorts the frame in
 * one workgroup). */
typedef struct aar_tracker_gate_params {
    uint32_t struct_size;
    double k_median;             /* t = max(min_px, k_median * median); <= 0: t = min_px */
    double min_px;
    int32_t min_detections;      /* frames with fewer detections are not gated */
} aar_tracker_gate_params;
typedef struct aar_tracker_gate_info {
    uint32_t struct_size;
    int32_t gated;               /* 0: the frame had fewer than min_detections detections, everything was kept */
    int32_t n_in, n_kept, n_nonfinite;
    double median, max, threshold;
} aar_tracker_gate_info;
void aar_tracker_default_gate_params(aar_tracker_gate_params *);   /* struct_size set; k_median 6, min_px 3, min_detections 4 (choices) */
/* Host function (no device needed): AAR_ERR_INVALID, the message naming the field, for a struct_size that does not reach min_detections, a
 * non-finite or negative min_px, a non-finite k_median, k_median and min_px both <= 0, min_detections < 1. */
int aar_tracker_gate_params_validate(const aar_tracker_gate_params *);
/* Once after aar_tracker_create or aar_tracker_reset, before the first push; again without a reset, or after a push: AAR_ERR_INVALID.
 * aar_tracker_reset forgets it.  Independent of aar_tracker_enable_detections; gates aar_tracker_push and aar_tracker_push_detections alike. */
int aar_tracker_enable_gate(aar_tracker *, const aar_tracker_gate_params *);
/* The gate record of the last accepted push, from its one copy back (no device work).  AAR_ERR_INVALID before any push, after a reset, or
 * without a gate. */
int aar_tracker_last_gate(aar_tracker *, aar_tracker_gate_info *out);
/* e_d and the keep flags of the newest frame in the order the caller pushed them: *n = n_in, det_err / keep: room for max_obs_per_frame
 * entries, either may be NULL.  The one call that makes a second device -> host copy. */
int aar_tracker_gate_detail(aar_tracker *, int32_t *n, double *det_err, uint8_t *keep);
/* The same for a bank (aar_tracker_bank_*): one parameter set for all members; the gate is ONE launch of B workgroups per push.  (The three are
 * named aar_tracker_gate_bank_*: the set of aar_tracker_bank_* symbols is pinned by tests/test_live_bank_host.py.) */
int aar_tracker_gate_bank_enable(aar_tracker_bank *, const aar_tracker_gate_params *);
int aar_tracker_gate_bank_last(aar_tracker_bank *, int32_t member, aar_tracker_gate_info *out);
int aar_tracker_gate_bank_detail(aar_tracker_bank *, int32_t member, int32_t *n, double *det_err, uint8_t *keep);

/* Constant-velocity motion model of the live tracker.  Off by default: a tracker that never enables it (or enables
 * AAR_TRACKER_MOTION_RANDOM_WALK) runs the kernels, copies the bytes and gives the bits described above.  With the model every pair keeps the
 * form of aar_track_smooth,
 *       e_f = [ log((R_f dR_f)^T R_{f+1}) ; t_{f+1} - t_f - dt_f ],   L_f unchanged,
 * and the pair that ENDS at pushed frame n carries an expected motion rel_n = (dR_n, dt_n) as (rvec, t):
 *   measured  once, when frame n is pushed, from the two newest estimates as push n - 1 left them (frames a = n - 2 and b = n - 1; with lag 0
 *             frame a is the anchor): omega = log(R_a^T R_b), v = t_b - t_a, s = (time_n - time_b) / (time_b - time_a), rel_n = (s omega, s v) --
 *             constant angular velocity in the body frame, constant linear velocity in the root camera's frame, the convention of e_f
 *   zero      for n < 2, and when max_dt > 0 and either of the two gaps exceeds max_dt (no coasting across a hole in the recording)
 *   lifetime  rel_n stays with frame n: it serves the window pair, the anchor pair once n - 1 is the anchor, and pair (0, 1) in the
 *             marginalisation and the covariance of AAR_TRACKER_ANCHOR_MARGINAL / covariance = 1.  It is never measured again.
 *   start     wherever the text above says "the current estimate of the previous frame", the new frame starts from the prediction
 *             (R_b exp(s omega), t_b + s v) instead; a pose_init still wins, and rel_n is measured from the estimates either way.
 * sigma_rot and sigma_trans then bound the deviation from CONSTANT VELOCITY per sqrt(unit of frame_time), no longer the motion itself.  rel_n is
 * an estimate fed back as a prior and frozen when measured -- the "relative motions of a previous pass" of aar_smooth_params.rel_motion -- which
 * keeps the system block tridiagonal; a second-difference prior would not.  The expected motions and the prediction are formed on the host in fp64
 * and travel in the kernel arguments and in the slot header: a push with the model makes the launches and copies of the same push without it.
 * Independent of aar_tracker_enable_detections and aar_tracker_enable_gate: AAR_TRACKER_START_BEST compares the vote with the prediction
 * (aar_tracker_start_info.start_source = 3 where it wins), the gate takes e_d there.  A tracker bank takes the model through
 * aar_tracker_motion_bank_*: one parameter set, every member its own expected motions and prediction; member b stays exactly an aar_tracker
 * with the model, and a bank push keeps its launches and its one copy each way (the copy in then carries 48 bytes per member more). */
#define AAR_TRACKER_MOTION_RANDOM_WALK 0
#define AAR_TRACKER_MOTION_CONSTANT_VELOCITY 1
typedef struct aar_tracker_motion_params {
    uint32_t struct_size;
    int32_t model;               /* AAR_TRACKER_MOTION_* */
    double max_dt;               /* >= 0 finite, in units of frame_time; 0 = no limit */
} aar_tracker_motion_params;
typedef struct aar_tracker_motion_info {
    uint32_t struct_size;
    int32_t model, predicted;    /* predicted: the rule measured rel for this push (n >= 2 and no gap above max_dt) */
    double rel[6];               /* the expected motion this push used (zeros when not predicted) */
    double velocity[6];          /* (omega, v) per unit of frame_time of the newest pair at the final point; zeros before two frames */
    double newest_time;
} aar_tracker_motion_info;
void aar_tracker_default_motion_params(aar_tracker_motion_params *);   /* struct_size set; AAR_TRACKER_MOTION_CONSTANT_VELOCITY, max_dt 0 */
/* Host function (no device needed): AAR_ERR_INVALID, the message naming the field, for a struct_size that does not reach model, an unknown
 * model, a negative or non-finite max_dt, and AAR_TRACKER_MOTION_CONSTANT_VELOCITY with smooth = 0 (there is no prior to carry it). */
int aar_tracker_motion_params_validate(const aar_tracker_params *, const aar_tracker_motion_params *);
/* Once after aar_tracker_create or aar_tracker_reset, before the first push; again without a reset, or after a push: AAR_ERR_INVALID.
 * aar_tracker_reset forgets it.  AAR_TRACKER_MOTION_RANDOM_WALK is accepted and leaves the tracker as if the call were not made. */
int aar_tracker_enable_motion(aar_tracker *, const aar_tracker_motion_params *);
/* The motion record of the last accepted push, from its one copy back (no device work).  AAR_ERR_INVALID before any push, after a reset, or
 * without the model.  A rejected push leaves it as it was. */
int aar_tracker_last_motion(aar_tracker *, aar_tracker_motion_info *out);
/* Host math: the newest pose (R_n, t_n) of the last accepted push carried to time >= newest_time with that push's velocity,
 * (R_n exp((time - t_n) omega), t_n + (time - t_n) v) as (rvec, t); the newest pose itself when max_dt > 0 and time - newest_time > max_dt.
 * AAR_ERR_INVALID for an earlier or non-finite time, before any push, or without the model.  The pose only: no covariance is propagated. */
int aar_tracker_predict(aar_tracker *, double time, double pose[6]);
/* The same for a bank: one parameter set for all members, enabled once after aar_tracker_bank_create or aar_tracker_bank_reset, before the first
 * push (aar_tracker_bank_reset forgets it); the record and the prediction of one member.  A rejected bank push leaves every member's motion state
 * as it was.  (Named aar_tracker_motion_bank_*: the set of aar_tracker_bank_* symbols is pinned by tests/test_live_bank_host.py.) */
int aar_tracker_motion_bank_enable(aar_tracker_bank *, const aar_tracker_motion_params *);
int aar_tracker_motion_bank_last(aar_tracker_bank *, int32_t member, aar_tracker_motion_info *out);
int aar_tracker_motion_bank_predict(aar_tracker_bank *, int32_t member, double time, double pose[6]);

#ifdef __cplusplus
}
#endif
#endif
