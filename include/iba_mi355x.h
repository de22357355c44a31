/*
 * iba_mi355x.h — C ABI of the MI355X-native IBA cross-modality evaluation path.
 *
 * This is the drop-in boundary for ONE hot path of
 * gitouni/Spatial-Temporal-LiDAR-camera-Calibration: the per-candidate-extrinsic
 * evaluation that the reference runs on the CPU in
 *   BAError()            src/examples/iba_global.cpp:169-344  (= iba_func.cpp:179-354)
 *   BALoss::eval_x()     src/examples/iba_global.cpp:377-396
 *   BuildProblem()       src/examples/iba_local.cpp:145-323   (association for the Jacobian path)
 *   IBA_PlaneFactor / Point2Point_Factor / Point2Plane_Factor
 *                        include/IBACalib2.hpp:152-184, 570-584, 611-625 (g2o twin: IBACalib.hpp:103-140)
 *
 * Only PODs cross the boundary: no Eigen / OpenCV / ORB_SLAM2 / torch types.
 * All pointers in iba_problem_desc are HOST pointers borrowed for the duration
 * of iba_create() only. Errors are return codes (the reference throws or
 * returns DBL_MAX sentinels; the sentinels are kept, see iba_cost_out).
 * A handle is thread-compatible: one evaluation at a time per handle
 * (BALoss::eval_x is called from NOMAD's single worker thread, iba_global.cpp:385).
 */
#ifndef IBA_MI355X_H
#define IBA_MI355X_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define IBA_ABI_VERSION 4 /* 2: iba_params.factor_3d2d_kind; 3: iba_icp_*; 4: iba_scan_*. An ADDED entry point (iba_submap_*, iba_lattice_*, iba_sc_*, iba_floam_*) changes no existing struct and does not bump it: callers detect it by symbol */
#define IBA_MAX_BATCH 64 /* the batch unit of the callers in this library (one MADS poll block, the planner's diagnostics); NOT a limit of the evaluators */
#define IBA_MAX_CHAIN 512 /* most candidates ONE launch chain takes (iba_create_options.max_chain_batch <= this); a call with more runs as consecutive chains */

typedef enum iba_status {
    IBA_OK = 0,
    IBA_ERR_INVALID_ARG = 1,
    IBA_ERR_NO_DEVICE = 2,   /* no gfx950 device / HIP runtime unusable: there is NO CPU fallback */
    IBA_ERR_HIP = 3,
    IBA_ERR_UNSUPPORTED = 4, /* problem shape outside what the kernels handle */
    IBA_ERR_STATE = 5,       /* e.g. iba_eval_factors before iba_build_problem */
    IBA_ERR_IO = 6           /* a dataset file is missing, truncated or not in the reference's format */
} iba_status;

typedef struct iba_handle iba_handle;

/*
 * Flat description of what the reference holds in
 *   std::vector<VecVector3d> PointClouds, std::vector<Eigen::Isometry3d> vTwl,
 *   std::vector<ORB_SLAM2::KeyFrame*> KeyFrames          (iba_global.cpp:169-173)
 * Frames are the keyframes sorted by mnId (iba_global.cpp:507). CSR offsets are
 * element counts (not bytes).
 */
typedef struct iba_problem_desc {
    int32_t n_frames; /* F */

    /* PointClouds[Fi] — raw scan in the LiDAR frame, float32 as in KITTI .bin (io_tools.h:170-187). */
    const uint64_t* pt_offset; /* [F+1] */
    const float* pts_xyz;      /* [N*3] AoS x,y,z */

    /* pKF->fx, fy, cx, cy, mnMaxX (W), mnMaxY (H)  (iba_global.cpp:64-65) */
    const double* intrinsics; /* [F*6] */

    /* pKF->mvKeysUn[i].pt (cv::Point2f) */
    const uint64_t* kp_offset; /* [F+1] */
    const float* kp_uv;        /* [K*2] */

    /* mapKpt2Mpt (inverse of pKF->mmapMpt2Kpt, iba_global.cpp:210-213):
     * MapPoint::GetWorldPos() (CV_32F 3x1) of the MapPoint owned by keypoint i. */
    const uint8_t* kp_has_mappoint; /* [K] 0/1 */
    const float* kp_mappoint_w;     /* [K*3] world position, ignored where kp_has_mappoint==0 */

    /* pKF->GetPoseSafe() (CV_32F 4x4, top 3 rows, row-major) */
    const float* Tcw; /* [F*12] */

    /* pKF->GetBestCovisibilityKeyFramesSafe(num_best_covis) (or ByWeight), iba_global.cpp:254-258.
     * One "slot" per (reference KF, covisible KF) pair; at most 62 per reference KF (30 match bits in the keypoint's flag word, a
     * second word for the slots beyond them; more: IBA_ERR_UNSUPPORTED). */
    const uint64_t* covis_offset; /* [F+1] slots of frame f are covis_offset[f]..covis_offset[f+1] */
    const int32_t* covis_frame;   /* [S] frame index of the covisible KF */
    /* pKFConv->GetPose() * InvRefCVPose evaluated in CV_32F (iba_global.cpp:280), top 3 rows
     * row-major, translation NOT multiplied by scale. */
    const float* covis_relpose; /* [S*12] */
    /* pKF->GetUordMatchedKptIds(pKFConv): keypoint id in the reference KF -> keypoint id in
     * the covisible KF (KeyFrame.cc:528-538 semantics). */
    const uint64_t* match_offset;  /* [S+1] */
    const int32_t* match_kp_ref;   /* [M] */
    const int32_t* match_kp_covis; /* [M] */

    /* Hand-eye term inputs (iba_global.cpp:264-276), one per frame, ignored for the last frame:
     *   Tc_next[f] = KeyFrames[f+1]->GetPose() * InvRefCVPose   in CV_32F, unscaled (:267)
     *   Tl_next[f] = vTwl[f+1].inverse() * vTwl[f]              double            (:269) */
    const float* Tc_next;  /* [F*12] */
    const double* Tl_next; /* [F*12] */
} iba_problem_desc;

/*
 * Thresholds. Field names follow IBAGlobalParams (iba_global.cpp:26-52) for the cost path
 * and IBALocalParams (IBACalib2.hpp:108-137) for the Jacobian path ("local_" prefix where the
 * two structs share a name but are configured independently).
 */
typedef struct iba_params {
    /* shared association (FindProjectCorrespondences) */
    double max_pixel_dist; /* 1.5 */

    /* cost path: BAError */
    int32_t num_min_corr_cost;   /* 30, hard-coded at iba_global.cpp:203 */
    double corr_3d_2d_threshold; /* 40 */
    double corr_3d_3d_threshold; /* 5 (yml: 10) */
    int32_t norm_max_pts;        /* 30 (<= 64 supported: the neighbour list lives one entry per lane of a wave) */
    int32_t norm_min_pts;        /* 5 */
    double norm_radius;          /* 0.6 */
    double norm_reg_threshold;   /* 0.04 (yml: 0.02) */
    double min_diff_dist;        /* 0.01 (yml: 0.2) */
    double err_weight[2];        /* {1,1} */
    int32_t use_plane;           /* 1 */

    /* Jacobian path: BuildProblem + Ceres losses */
    int32_t num_min_corr;             /* 30 */
    double max_3d_dist;               /* 1.0 */
    double neigh_radius;              /* 0.6 */
    int32_t neigh_max_pts;            /* 30 (<= 64 supported) */
    int32_t neigh_min_pts;            /* 5 */
    double local_min_diff_dist;       /* 0.2 */
    double local_norm_reg_threshold;  /* 0.001 */
    double robust_kernel_delta;       /* 2.98 */
    double robust_kernel_3ddelta;     /* 1.0 */

    /* engine knob (no reference counterpart): 1 = memoise the x-independent local-plane fit per
     * scan point (bit-identical results); 0 = refit inside every evaluation as the reference does. */
    int32_t plane_cache;

    /* Which 3d-2d residual the Jacobian path builds (ABI version 2):
     *   0  IBA_PlaneFactor (IBACalib2.hpp:152-184; g2o twin IBAPlaneEdge, IBACalib.hpp:103-140): the keypoint's ray intersected with the
     *      local plane at its scan point, reprojected into every covisible keyframe — one block of 2 NConv rows per keypoint [default];
     *   1  IBATestEdge (IBACalib.hpp:14-71, functor :40-58): the DIRECT point-to-pixel term — the matched scan point itself,
     *      p1 = R_i (R_cl p0 + t_cl) + s t_i, one 2-row block per (correspondence, matched covisible keyframe), Huber(robust_kernel_delta)
     *      each. The reference declares the edge and instantiates it nowhere; the edge set here is that of BAError's 3d-2d loop
     *      (iba_global.cpp:291-328: every correspondence of a used frame x every covisible keyframe that matches its keypoint; no plane, no
     *      MapPoint, no neighbourhood test), whose cost these are the normal equations of. The 3d-3d blocks are built as in mode 0 when
     *      err_weight[1] > 1e-10 and not at all otherwise (BAError's switch, :214-220): err_weight = {1, 0} is BASELINE's
     *      "point-to-pixel only" configuration on the Jacobian path. Mode 1 is an EXTENSION without a reference-run counterpart: the
     *      reference never constructs the edge, so there is no reference output to validate against (it is checked against the oracle's
     *      restatement of the functor and an independent autograd evaluation only), and its cost follows this library's Ceres convention
     *      (0.5 rho) although the edge's reference twin is a g2o edge. */
    int32_t factor_3d2d_kind;
} iba_params;

/* GeoCalib.h:18-33 computeCorrespondence, the cloud-to-cloud 1-NN correspondence north_star's "GeoCalib call surface" names: for every
 * source point the nearest target point (nanoflann KDTreeSingleIndexAdaptor, L2_Simple, max_leaf 15: the leaf size does not change a result),
 * kept when  sq_dist <= max_distance  — the SQUARED distance against the un-squared parameter, exactly as the reference writes it (:29);
 * pairs (source index, target index) in ascending source order (:30).
 * The target cloud is the scan of local keyframe `frame` of the handle (the float32 points as loaded, io_tools.h:170-187; indices are the scan's
 * ORIGINAL order), searched by the kd search of the evaluation path itself (exact f64 distances; a tie between two target points goes to the
 * lower index, nanoflann keeps the first visited: only duplicate points can tie). src_xyz: n_src points (x, y, z doubles) in that scan's frame —
 * the caller applies its transform, as computeInitialGeoError does (GeoCalib.h:76-105). out_src / out_tgt: room for n_src entries each.
 * The header is an orphan of the reference (nothing includes it, and std::vector<Eigen::Vector3d> is no nanoflann dataset: it does not compile
 * there); this entry point exists so that the one name north_star lists is not missing, and is pinned against the reference's own nanoflann. */
iba_status iba_geo_correspondences(iba_handle* h, int32_t frame, const double* src_xyz, int32_t n_src, double max_distance,
                                   uint32_t* out_src, uint32_t* out_tgt, int32_t* n_out);

/*
 * ---- Scaled point-to-point ICP on the device kd search [SURVEY.md 2 row 18: icp_calib.cpp:10-86, the geometry-only ablation baseline] ----
 * icp_calib registers the ORB map cloud (source) to the LiDAR map cloud (target) with Open3D's RegistrationICP and
 * TransformationEstimationPointToPoint(true), starting from the hand-eye Sim(3), and writes a Sim(3). Open3D is not part of the reference
 * tree: the loop is RESTATED here from its public sources and its parity is UNPINNED (the kd search underneath stays pinned to the reference's
 * nanoflann). What is restated:
 *   RegistrationICP                              evaluate at init; up to max_iter times: update = estimation(correspondences), T = update * T,
 *                                                re-evaluate, stop when |d fitness| < relative_fitness AND |d inlier_rmse| < relative_rmse
 *   GetRegistrationResultAndCorrespondences      per source point the nearest target point inside the gate; fitness = kept / n_src,
 *                                                inlier_rmse = sqrt(sum d^2 / kept) (both 0 when nothing is kept)
 *   KDTreeFlann::SearchHybrid(query, r, 1)       a k = 1 search followed by lower_bound(d^2, r^2): a pair is kept when d^2 < r^2, STRICTLY
 *                                                (iba_geo_correspondences, GeoCalib.h:29, keeps d^2 <= its parameter)
 *   Eigen::umeyama(src, dst, with_scaling)       sigma = 1/n sum (p - mean_p)(q - mean_q)^T = U D V^T; S = diag(1, 1, -1) when
 *                                                det(U) det(V) < 0; R = U S V^T; c = tr(D S) / var_q (1 without scaling); t = mean_p - c R mean_q
 * Two deviations, both known: (1) Open3D transforms its working copy of the source cumulatively, one more rounding per point and iteration;
 * here the composed T is applied to the ORIGINAL source points in every pass (one rounding, whatever the iteration). (2) Between two target
 * points at exactly the same distance the lower (frame, index) wins, the tie rule of the kd search; FLANN keeps the first it visits.
 *
 * Target cloud: the scans of local frames [frame_begin, frame_end) of the handle, read as TILES of one cloud in one coordinate frame (a
 * scans-only handle is enough). A target point is the pair (local frame, original index in that scan). frame_end - frame_begin == 1 is the
 * common case and runs the single search; with more tiles a lane searches them in ascending order, carries its best distance into the next
 * tile's search and skips a tile whose bounding box lies further away than that. No limit on the tiles but the handle's frames; a tile holds
 * what a scan holds.
 * Source cloud: n_src points (x, y, z doubles). q = T x is evaluated in f64, row r as fma(T[r][2], z, fma(T[r][1], y, fma(T[r][0], x, T[r][3])))
 * (the library is built without floating-point contraction: exactly these three operations fuse). T: row-major 4x4, rows 0-2 are read.
 *
 * Moments of one pass (iba_icp_step; IBA_ICP_NMOM doubles per transform), summed on the device over the kept pairs (q, p), p the target point,
 * about the PIVOT v = T * centroid(source) (centroid: plain sequential f64 mean of src_xyz on the host), dq = q - v, dp = p - v:
 *   [0] kept pairs   [1] sum d^2 (d^2 = ((qx-px)^2 + (qy-py)^2) + (qz-pz)^2, the search's own value)   [2..4] sum dq   [5..7] sum dp
 *   [8] sum |dq|^2   [9..17] sum dp dq^T, row-major (entry 9 + 3 i + j = sum dp_i dq_j)   [18..20] the pivot v
 * The sums have a fixed order (a wave's 64 lanes by DPP, the waves of a transform by position): two calls give the same bits, and a
 * transform's block does not depend on what else is in the batch. No atomics on floating-point values.
 */
#define IBA_ICP_NMOM 21
#define IBA_ICP_CONVERGED 1      /* iba_icp_result.converged: both criteria met */
#define IBA_ICP_MAX_ITER 0       /* max_iter updates applied (max_iter = 0: evaluation only) */
#define IBA_ICP_DEGENERATE (-1)  /* fewer than 3 kept pairs, or a source set without spread: no update is defined; T is the last valid one */
typedef struct iba_icp_options {
    int32_t struct_size;
    double  max_corr_dist;      /* icp_calib.cpp:26; a pair is kept when d^2 < max_corr_dist^2 (strict) */
    int32_t max_iter;           /* icp_calib.cpp:27,62 */
    double  relative_fitness;   /* Open3D ICPConvergenceCriteria defaults: 1e-6 */
    double  relative_rmse;      /* 1e-6 */
    int32_t with_scaling;       /* 1 = TransformationEstimationPointToPoint(true), what icp_calib uses; 0 = rigid */
} iba_icp_options;
typedef struct iba_icp_result {
    double  T[16];              /* row-major 4x4, source -> target, upper-left block = c * R */
    double  scale;              /* c = sqrt((A A^T)_00) of the upper-left block A */
    double  fitness;            /* kept pairs / n_src */
    double  inlier_rmse;        /* sqrt(sum d^2 / kept pairs) */
    int32_t n_corr, iterations, converged;   /* iterations: updates applied; converged: IBA_ICP_* */
} iba_icp_result;
/* max_corr_dist 1.0, max_iter 30 (Open3D's default), 1e-6, 1e-6, with_scaling 1 */
iba_status iba_default_icp_options(iba_icp_options* opt);
/* One correspondence pass per transform (GeoCalib.h computeCorrespondenceList: one tree, B clouds that are transforms of one cloud, one launch
 * chain). pair_frame / pair_idx: both NULL (nothing of size n_src leaves the device) or B x n_src entries each: the target of every source
 * point, 0xFFFFFFFF in both where the pair is not kept. B in [1, 4096]; n_src = 0 answers zero moments. */
iba_status iba_icp_step(iba_handle* h, int32_t frame_begin, int32_t frame_end, const double* src_xyz, int32_t n_src,
                        const double* T /* B x 16 */, int32_t B, double max_corr_dist, double* moments /* B x IBA_ICP_NMOM */,
                        uint32_t* pair_frame, uint32_t* pair_idx);
/* RegistrationICP from B independent starts. The source is uploaded once and stays on the device; per iteration the transforms of the starts
 * still running go down and their moment blocks come back. The 3x3 Umeyama runs on the host. A start's result does not depend on the batch. */
iba_status iba_icp_register(iba_handle* h, int32_t frame_begin, int32_t frame_end, const double* src_xyz, int32_t n_src,
                            const double* T_init /* B x 16 */, int32_t B, const iba_icp_options* opt, iba_icp_result* out /* B */);
/* icp_calib.cpp:43-71 around the loop: iba_read_sim3 -> this -> iba_write_sim3 is the program (PCD reading is the caller's: clouds are arrays).
 * (rigid12_init, scale_init) in readSim3 form is inverted (R^T, -R^T t) and its rotation multiplied by the scale (:55-60); the result's
 * scale is sqrt((A A^T)_00) of its upper-left block, the block is divided by it and the transform inverted back (:67-71).
 * ref_lidar_pose12 (NULL: none): the LiDAR pose of the camera reference frame, lidar_poses[FrameId[0]] (:43-51). The reference moves the
 * LiDAR cloud by refpose^-1; here the stored scans stay untouched and the QUERIES are moved instead — the registration runs from
 * refpose * init and its result is multiplied by refpose^-1: the same registration in another frame (distances do not change). */
iba_status iba_icp_calib(iba_handle* h, int32_t frame_begin, int32_t frame_end, const double* cam_xyz, int32_t n,
                         const double rigid12_init[12], double scale_init, const double* ref_lidar_pose12,
                         const iba_icp_options* opt, double rigid12_out[12], double* scale_out, iba_icp_result* res);

/*
 * ---- Batched scan-to-scan ICP edges: point-to-point, point-to-plane, information matrix [SURVEY.md 2 row 16: backend_opt.cpp:27-45 Registration,
 * :64-82 PLRegistration, :446-511 MultiRegistration; GeoCalib.h:76-105] ----
 * The reference's LiDAR back end registers keyframe scans against each other: for every odometry edge (i-1, i) and every loop edge it takes
 * relPose = pose[j] * pose[i]^-1 (:158-161), optionally refines it with Open3D's RegistrationICP (one stage or coarse -> refine) and attaches
 * GetInformationMatrixFromPointClouds(src, tgt, MRmaxCorrDist, T). Here a BATCH OF EDGES between local frames of one handle is evaluated
 * together: per ICP iteration one launch chain and one synchronise for all edges still running, and nothing of scan size crosses PCIe —
 * source and target scans, the target's kd tree and its memoised normals are already resident. A scans-only handle is enough.
 * Voxel down-sampling and the merged sub-map target of a loop closure are iba_submap_build, and choosing WHICH keyframe pairs to close a loop between
 * (Scan Context) is iba_sc_describe / iba_sc_detect (both below); the pose-graph optimisation over the resulting edges is iba_pgo_* (below:
 * Open3D's GlobalOptimization), the smoothing stage that yields the isam poses is iba_smooth_* with the plan of iba_backend_plan (both below; GTSAM's
 * iSAM2 is restated as its converged optimum, not linked), and PCD IO stays the caller's.
 *
 * Restated from Open3D's public sources (not part of the reference tree: parity with it is UNPINNED; the kd search stays pinned to nanoflann):
 *   RegistrationICP, GetRegistrationResultAndCorrespondences, SearchHybrid's strict gate    the loop of iba_icp_register (one implementation)
 *   TransformationEstimationPointToPoint(false)     Eigen::umeyama without scaling on the pivoted sums (as iba_icp_*, with_scaling = 0)
 *   TransformationEstimationPointToPlane            per kept pair (q = T x, target point p, unit normal n of p): r = (q - p) . n,
 *                                                   J = [q x n, n]; JtJ x = -Jtr solved on the host (6x6 LDL^T); update = Rz(x2) Ry(x1) Rx(x0)
 *                                                   with translation x[3..5] (TransformVector6dToMatrix4d); T = update * T
 *   GetInformationMatrixFromPointClouds             over the pairs kept at max_dist under T, t the TARGET point: sum G^T G, G's rows
 *                                                   [0, tz, -ty, 1, 0, 0], [-tz, 0, tx, 0, 1, 0], [ty, -tx, 0, 0, 0, 1] (row-major 6x6 out)
 * Rules fixed here:
 *   * Normals: the cost path's plane memo (iba_params.norm_radius / norm_max_pts; plane_cache = 1), the analogue of
 *     EstimateNormals(KDTreeSearchParamHybrid(r, 30)). A target point whose record kept fewer than max(norm_min_pts, 3) neighbours (or whose
 *     normal is not finite) has NO normal: a pair on it stays in fitness / inlier_rmse (inside the gate) and adds nothing to JtJ / Jtr;
 *     n_planar counts the pairs that carried one. Point-to-plane does not depend on the sign of n: no orientation step.
 *   * A point-to-plane update is defined with at least 6 pairs that carry a normal and a system whose LDL^T pivots are positive, finite and,
 *     within the rotation and the translation block each, not below 1e-12 of the block's largest (a scene of parallel planes fails this);
 *     otherwise the edge ends IBA_ICP_DEGENERATE with the last valid T. (Open3D tests the determinant instead; unpinned.)
 *   * Coarse -> refine: the refine stage starts from the coarse stage's T (backend_opt.cpp:36-44); the result is the refine stage's.
 *   * backend_opt.cpp:31,39,43 pass the correspondence DISTANCE as the third argument of ICPConvergenceCriteria, which is (as its public
 *     signature is remembered: relative_fitness, relative_rmse, max_iteration) the ITERATION COUNT: config/loam/backend.yml (icp_corase_dist
 *     1.0, icp_refine_dist 0.3) thereby asks for 1 coarse iteration and 0 refine iterations. This API takes the counts explicitly
 *     (INTEGRATION.md names the values that reproduce the call as written).
 *   * Known deviations, as for iba_icp_*: the composed T is applied to the original source points in every pass; distance ties go to the
 *     lowest index; the source points are the scan's float32 values widened to double.
 * Sums of one pass (iba_scan_step; IBA_SCAN_NMOM doubles per edge, unused entries 0), in a fixed order (one partial per 64 positions of the
 * source scan in kd-tree order, a wave's lanes by DPP, the partials of an edge by position): two calls give the same bytes and an edge's block
 * does not depend on the batch. No floating-point atomics.
 *   IBA_SCAN_POINT_TO_POINT   the layout of IBA_ICP_NMOM ([0] pairs, [1] sum d^2, .. [18..20] pivot), the pivot = T * centre of the source
 *                             scan's bounding box
 *   IBA_SCAN_POINT_TO_PLANE   [0] pairs  [1] sum d^2  [2] pairs with a normal  [3..23] JtJ, upper triangle by rows  [24..29] Jtr  [30] sum r^2
 *   IBA_SCAN_INFORMATION      [0] pairs  [1..3] sum t  [4..9] sum t t^T (xx, xy, xz, yy, yz, zz)
 * The point-to-plane and information sums are taken about the origin of the target frame, as the definitions are.
 * Limits: one target scan per edge; rigid only (the scaled form is iba_icp_*); no robust kernel; one GPU — both frames of an edge are
 * local frames of this handle. The reference registers voxel clouds, never raw scans: iba_submap_handle (below) gives a handle whose frames
 * ARE voxel clouds, built on the device, and every entry point of this block runs on it unchanged.
 */
typedef struct iba_scan_edge { int32_t src_frame, tgt_frame; double T[16]; } iba_scan_edge; /* row-major 4x4, src scan frame -> tgt scan frame */
#define IBA_SCAN_POINT_TO_POINT 0   /* TransformationEstimationPointToPoint(false) */
#define IBA_SCAN_POINT_TO_PLANE 1   /* TransformationEstimationPointToPlane() */
#define IBA_SCAN_INFORMATION 2      /* iba_scan_step only: the sums of the information matrix */
#define IBA_SCAN_NMOM 32
typedef struct iba_scan_options {
    int32_t struct_size, estimation;
    double  coarse_dist;        /* <= 0: one stage (refine only) */
    int32_t coarse_max_iter;
    double  coarse_rel_fitness, coarse_rel_rmse;
    double  refine_dist;
    int32_t refine_max_iter;    /* 0: evaluation only */
    double  refine_rel_fitness, refine_rel_rmse;
    double  info_dist;          /* <= 0: no information matrix */
} iba_scan_options;
typedef struct iba_scan_result {
    iba_icp_result reg;         /* of the last stage; scale is 1 up to rounding */
    int32_t n_planar;           /* point-to-plane: pairs of the last evaluation that carried a normal (0 under point-to-point) */
    double  info[36];           /* row-major 6x6 at reg.T (zeros without info_dist) */
    int32_t n_info;             /* pairs kept at info_dist */
} iba_scan_result;
/* point-to-point, one stage: refine 0.3 m, 30 iterations, 1e-6, 1e-6 (Open3D's defaults); coarse off (dist 0; 30, 1e-4, 1e-4 once enabled); info off */
iba_status iba_default_scan_options(iba_scan_options* opt);
/* One correspondence pass per edge. E in [1, 4096]. pair_idx: NULL, or sum over the edges of P(src_frame) entries, edge after edge, each
 * edge's block in the ORIGINAL point order of its source scan: the original index of the target point, 0xFFFFFFFF = not kept.
 * IBA_ERR_INVALID_ARG with a message, before any launch: a frame outside the handle, src_frame == tgt_frame, a non-finite T, point-to-plane
 * on a handle with plane_cache = 0. An edge with an empty source or target scan answers zero sums. */
iba_status iba_scan_step(iba_handle* h, const iba_scan_edge* edges, int32_t E, double max_corr_dist, int32_t estimation,
                         double* moments /* E x IBA_SCAN_NMOM */, uint32_t* pair_idx);
/* RegistrationICP per edge from edges[e].T, all edges together. An edge with an empty scan comes back as it is, IBA_ICP_DEGENERATE. */
iba_status iba_scan_register(iba_handle* h, const iba_scan_edge* edges, int32_t E, const iba_scan_options* opt, iba_scan_result* out /* E */);
/* GetInformationMatrixFromPointClouds per edge at edges[e].T */
iba_status iba_scan_information(iba_handle* h, const iba_scan_edge* edges, int32_t E, double max_dist, double* info /* E x 36 */, int32_t* n_pairs /* E */);

/*
 * ---- Voxel down-sampling and merged sub-map clouds [backend_opt.cpp:164-172 LoadPCD, :174-185 MergeLoadPCD, target of every loop closure :259-262] ----
 * The reference passes every keyframe scan through VoxelDownSample(voxel) (LoadPCD) and builds the target of a loop-closure registration from the
 * 2 x LCSubmapSize scans around the history frame: each transformed by its pose, concatenated, VoxelDownSample(voxel), moved into the history
 * frame by pose[ref]^-1 (MergeLoadPCD). Here a BATCH OF SUB-MAPS is built in one launch chain from scans that are already resident in the handle
 * (a scans-only handle is enough): only the pose / descriptor blocks go down and only the voxel clouds come up, nothing of input-scan size
 * crosses PCIe. A frame may be a member of many sub-maps and may appear twice in one. LoadPCD = the one-member sub-map with the identity pose
 * and out12 = NULL.
 *
 * Restated from Open3D's public PointCloud::Transform, operator+= and VoxelDownSample (Open3D is not part of the reference tree: parity with it is
 * UNPINNED). The rules, fixed here so that the result is a function of the input alone (tests/submap_ref.py restates them in numpy and the device
 * result is compared with it byte for byte):
 *   1 member point   the scan's float32 coordinates widened to double; q_r = ((T[r][0] x + T[r][1] y) + T[r][2] z) + T[r][3]: four separately
 *                    rounded f64 operations in exactly this order, NO fused multiply-add (deliberately unlike the fma chain of iba_icp_* / iba_scan_*:
 *                    voxel membership is a floor, so the restatement must reproduce q to the bit, and numpy has no fma). Known deviation: Eigen's
 *                    product in Transform may round differently. A point with a non-finite coordinate before or after the transform is DROPPED
 *                    and counted in n_dropped (Open3D would let it poison a voxel).
 *   2 bounds         minb = min over the kept q - 0.5 voxel per axis; index = floor((q - minb) / voxel) (IEEE f64 division, floor), Open3D's expression.
 *   3 accumulation   a voxel's point is (sum q) / double(count) per axis, the sum taken SEQUENTIALLY in concatenation order: members in list order,
 *                    the points of a member in the scan's ORIGINAL index order (Open3D's accumulator). The same bytes on every call, whatever
 *                    else is in the batch. No floating-point atomics.
 *   4 output         out12 (NULL: none) applied to every averaged point with the expression of rule 1.
 *   5 order          voxels in ascending (ix, iy, iz), lexicographic (Open3D's order is that of an unordered_map: unspecified).
 * Answers IBA_ERR_INVALID_ARG with a message, before any launch: a NULL argument, struct_size, n_members < 1, a frame outside the handle, a
 * non-finite pose or out12, voxel not finite or not > 0, M outside [1, 4096]. IBA_ERR_UNSUPPORTED: a sub-map whose kept points span more than
 * 2^17 = 131072 voxels along an axis (the sort key holds the sub-map and three 17-bit indices; known after the first kernel, before the sort),
 * more than 2^22 members or more than 2^32 - 256 member points in one call. A sub-map whose members hold no kept point answers zero voxels.
 * Limits: iba_submap_build brings the clouds back to the host; iba_submap_handle (below) keeps them on the device instead and makes them the
 * frames of a new handle — registration targets, Scan Context nodes, members of further sub-maps — whose normals are that handle's plane memo.
 * Clouds cannot be attached to an EXISTING handle. Loop detection is iba_sc_* and the pose graph iba_pgo_* (both below), PCD IO is not here; one GPU — the
 * members of a sub-map are local frames of one handle.
 */
typedef struct iba_submap_desc {
    int32_t struct_size;      /* sizeof(iba_submap_desc) */
    int32_t n_members;
    const int32_t* frames;    /* [n_members] local frames of the handle */
    const double*  poses12;   /* [n_members x 12] row-major 3x4, scan frame -> common frame */
    const double*  out12;     /* row-major 3x4 applied to the averaged points, or NULL (MergeLoadPCD: pose[ref]^-1) */
    double voxel;             /* backend.yml: voxel */
} iba_submap_desc;
typedef struct iba_submap_clouds iba_submap_clouds;
/* The result is allocated by the library (its size is not known up front); release it with iba_submap_free. *out is NULL on failure. */
iba_status iba_submap_build(iba_handle* h, const iba_submap_desc* subs, int32_t M, iba_submap_clouds** out);
/* Of a result: its sub-maps (0 for NULL); of sub-map s: voxels and dropped points (-1 for NULL or s out of range), the points as doubles
 * (x, y, z per voxel) and the points that went into each voxel (n_voxels entries each, valid until iba_submap_free; NULL for NULL or s out of range). */
int32_t iba_submap_num(const iba_submap_clouds* c);
int64_t iba_submap_n_voxels(const iba_submap_clouds* c, int32_t s);
int64_t iba_submap_n_dropped(const iba_submap_clouds* c, int32_t s);
const double* iba_submap_xyz(const iba_submap_clouds* c, int32_t s);
const int32_t* iba_submap_counts(const iba_submap_clouds* c, int32_t s);
void iba_submap_free(iba_submap_clouds* c);
/* A scans-only handle whose local frame s is the voxel cloud of sub-map s, built without the clouds leaving the device.
 * subs / M: the argument rules of iba_submap_build and its messages (headed by this function's name), checked before any launch; they are left
 * in iba_last_error(src). Frame s of *out holds exactly the points iba_submap_xyz(c, s) would return, each coordinate narrowed to float32 with
 * round-to-nearest-even (the C cast a caller of iba_create applies), original index = voxel order, ascending (ix, iy, iz). The kd index, the
 * leaf-ordered arrays and the boxes are built on the device (csrc/iba_index_kernels.hpp) and are BIT-IDENTICAL to what iba_create builds on the
 * host for the same float32 points, so every result on *out equals the result on such a handle. A sub-map without voxels is an empty frame
 * (edges on it answer as empty scans do). A coordinate that is not finite after narrowing, or a sub-map of 2^22 voxels or more:
 * IBA_ERR_UNSUPPORTED. *out lives on src's device, has its own stream, does not depend on src's lifetime and is released with iba_destroy; it
 * is NULL on failure. params: as for iba_create (plane_cache = 1 builds the plane memo, which point-to-plane edges need). The keypoint side
 * is empty: iba_scan_*, iba_icp_*, iba_geo_correspondences, iba_sc_describe, iba_submap_build / iba_submap_handle (a sub-map of sub-maps) and
 * the debug probes work on it. Up go the bounds and voxel counts per sub-map and 32 B of frame box per frame; nothing of cloud size crosses PCIe. */
iba_status iba_submap_handle(iba_handle* src, const iba_submap_desc* subs, int32_t M, const iba_params* params, iba_handle** out);

/*
 * ---- The lattice voxel filter with a crop box: PCL's VoxelGrid and CropBox as F-LOAM's local map uses them [src/floam/src/odomEstimationClass.cpp:
 * downSamplingToMap :94-99, addPointsToMap :210-250] ----
 * iba_submap_build's grid is Open3D's: it hangs on the cloud's own minimum, so the cells move whenever the cloud's extent does. A local map that is
 * filtered again after every scan needs PCL's rule — cells anchored at the ORIGIN, the same cells on every step — and a box that cuts the map to the
 * neighbourhood of the sensor. iba_lattice_build is that filter on the same inputs (resident scans + poses, a BATCH OF SUB-MAPS per launch chain) with
 * the same result object and accessors. The result is a function of the input alone (tests/floam_odom_ref.py restates the rules in numpy; the device
 * result equals it byte for byte):
 *   L1 point     rule 1 of iba_submap_build, unchanged: float32 widened to f64, four separately rounded operations, no fused multiply-add; members in
 *                list order, a member's points in original index order; a non-finite point is dropped and counted in n_dropped.
 *   L2 crop      with has_crop, a point is kept iff crop_lo[a] <= q[a] <= crop_hi[a] on all three axes, BOTH ends inclusive as PCL's CropBox is; the
 *                others are counted in n_cropped (a dropped point is never counted as cropped). KNOWN DEVIATION: PCL compares in float. The crop
 *                takes effect in the first kernel: a cropped point takes part in no bound and costs no sort key beyond the drop bucket.
 *   L3 cell      i[a] = floor(q[a] / leaf): IEEE f64 division, then floor; the origin is the anchor, there is no minb (floor(-0.1 / 0.4) = -1, and
 *                -0 lies in cell 0). KNOWN DEVIATION: PCL forms floor(float(q) * inv_leaf) in float. A sub-map whose kept points span more than
 *                2^17 cells along an axis (max i - min i + 1) answers IBA_ERR_UNSUPPORTED, with the wording of iba_submap_build's check.
 *   L4 centroid  rules 3-5 of iba_submap_build, unchanged: sequential f64 sums in concatenation order divided by double(count), out12 applied after,
 *                voxels ascending (ix, iy, iz), every occupied cell gives a point (PCL's min_points_per_voxel = 0). KNOWN DEVIATIONS: PCL
 *                accumulates in float after an unstable sort and orders by (iz, iy, ix).
 * Arguments: iba_submap_build's rules and messages, headed by this function's name (the cell size is named leaf); in addition crop_lo and crop_hi must
 * be finite with lo <= hi, whether or not has_crop is set. A sub-map emptied by the crop answers zero voxels.
 * Limits: the clouds come back to the host, as iba_submap_build's do; iba_floam_odom_run (further below) runs the same chain on the device without
 * the download to keep F-LOAM's local map. One GPU.
 */
typedef struct iba_lattice_desc {
    int32_t struct_size;      /* sizeof(iba_lattice_desc) */
    int32_t n_members;
    const int32_t* frames;    /* [n_members] local frames of the handle */
    const double*  poses12;   /* [n_members x 12] row-major 3x4, scan frame -> common frame */
    const double*  out12;     /* row-major 3x4 applied to the centroids, or NULL */
    double  leaf;             /* cell size (odomEstimationClass: map_resolution for edges, 2 x map_resolution for surfs) */
    int32_t has_crop;         /* 0: no crop (crop_lo / crop_hi must still be finite, lo <= hi: zeros do) */
    int32_t reserved;         /* 0 */
    double  crop_lo[3];       /* the box in the common frame, before out12 */
    double  crop_hi[3];
} iba_lattice_desc;
/* The result is read through the iba_submap_* accessors and released with iba_submap_free. *out is NULL on failure. */
iba_status iba_lattice_build(iba_handle* h, const iba_lattice_desc* subs, int32_t M, iba_submap_clouds** out);
/* Points of sub-map s that the crop box removed (rule L2); 0 for a result of iba_submap_build, -1 for NULL or s out of range. */
int64_t iba_submap_n_cropped(const iba_submap_clouds* c, int32_t s);

/*
 * ---- Scan Context: descriptors, ring keys, batched loop search [src/scancontext/Scancontext.cpp: makeScancontext(vector<Vector3d>) :198-240, ring / sector
 * keys :242-271, distDirectSC :70-91, fastAlignUsingVkey :94-114, distanceBtnScanContext :117-149, detectLoopClosureID :393-486; called per keyframe from
 * backend_opt.cpp:325,361 and :305] ----
 * The reference describes every keyframe scan by a num_ring x num_sector matrix of the highest z per polar bin, keeps its row means (ring key) and column
 * means (sector key), and asks per keyframe for the nearest older descriptor: 3 ring-key neighbours from a kd tree that is rebuilt every 30th call and
 * leaves out the 30 most recent keyframes, each compared by the column-cosine distance under the best of 7 column shifts; below 0.2 it is a loop, which
 * LoopClosureRegThread turns into a MergeLoadPCD target and a coarse -> refine registration. Scan Context depends on the scans alone, never on the
 * optimised poses: here the descriptors of a BATCH OF RESIDENT SCANS are built in one launch chain into a database that stays on the device
 * (iba_sc_describe; a scans-only handle is enough), and the whole detection sequence of a run is one batch of queries over it (iba_sc_detect).
 * iba_sc_replay_plan (host only) turns the reference's call sequence into those queries; iba_sc_replay_plan -> iba_sc_detect -> iba_submap_build ->
 * iba_scan_register is PerformLoopClosure + LoopClosureRegThread.
 *
 * Rules, fixed here so that the result is a function of the input alone (tests/sc_ref.py restates them in numpy; the device result is compared with it byte
 * for byte). Every f64 operation below is rounded on its own: NO fused multiply-add; sqrt and / are IEEE. No floating-point atomics anywhere.
 *   1 point      the scan's float32 coordinates widened to double. A point with a non-finite coordinate is SKIPPED and counted. zz = z + lidar_height;
 *                range = sqrt((x x + y y) + zz zz), the 3-D norm as the back end's overload takes it (not the xy range of the PCL overload);
 *                angle = atan2(y, x) * (180 / pi), + 360 when negative; x == 0 && y == 0 has angle 0 (the reference divides 0 / 0 there). Known
 *                deviation: the reference narrows range and angle to float and takes atan of a float quotient by quadrant; here both stay f64.
 *   2 bins       a point with range > max_radius is skipped; ring = max(min(num_ring, int(ceil(range / max_radius * num_ring))), 1), sector =
 *                max(min(num_sector, int(ceil(angle / 360 * num_sector))), 1): the reference's expressions. Range and ring are IEEE and reproduce to the
 *                bit; the f64 atan2 of two correct libraries may differ by a few ulp (about 1e-14 in bin units), which matters only for a point whose
 *                angle sits on a sector boundary. y == +-0 with x > 0 is exact (atan2 answers +-0: sector 1).
 *   3 bin value  the largest float32 z of the points that entered, widened, + lidar_height; an empty bin is 0. A point enters only with zz > -1000: the
 *                reference's strict '<' against its -1000 initial value, and its final pass turns -1000 into 0 (a real z of exactly -1000 is 0 too).
 *                On the device: integer atomic max on an order-preserving 32-bit key of the float32 z (+0 orders above -0), in LDS first, then global.
 *                A maximum does not depend on the order: the descriptor is exact once the bins agree.
 *   4 sums       ring key[r] = (sum over the sectors ascending) / num_sector; sector key[c] = (sum over the rings ascending) / num_ring; column norm[c]
 *                = sqrt(sum over the rings ascending of v v), computed once per descriptor (a shift does not change it); dot products rings ascending;
 *                the sum over the columns of a distance and over the sectors of an alignment ascending. The search takes the ring key narrowed to float.
 *                (Eigen's own reductions may associate differently: a known deviation in the last bits.)
 *   5 distance   alignment = the first shift in 0 .. num_sector - 1 that minimises |sector key 1 - circshift(sector key 2, shift)| (square root taken,
 *                compared with '<' from the reference's initial 10000000). SEARCH_RADIUS = round(0.5 * search_ratio * num_sector); the shifts within it
 *                of the alignment (mod num_sector) are tried ASCENDING; distance(shift) = 1 - (sum of dot / (norm1 * norm2) over the columns where both
 *                norms are non-zero) / their count, 0 / 0 = NaN without such a column; the first minimum under '<' wins. A NaN never wins: when no shift
 *                wins, the distance is the reference's initial 10000000 with shift 0.
 *   6 search     the num_candidates nearest ring keys by EXACT brute force over [0, db_end) on the float keys, f64 squared distances summed rings
 *                ascending, nearest first, equal distances to the lower node. Known deviation: nanoflann accumulates in float and keeps the first
 *                visited (the index SETS agree on the golden fixture tests/golden/sc_ringkey_nanoflann.npz). With db_end < num_candidates only the
 *                existing nodes are candidates and the other slots are -1 (node and shift) / NaN (distance): the reference reads uninitialised indices.
 *   7 detection  the candidates in search order, the first strict minimum from 10000000 wins; loop_node = that node when min_dist < dist_thres, else -1;
 *                yaw_rad = (float)(shift * (360.0 / num_sector) * M_PI / 180.0). A query's result does not depend on the batch, and two calls give
 *                the same bytes.
 * Answers IBA_ERR_INVALID_ARG with a message, before any launch: a NULL argument, a struct_size of another library, num_ring outside [1, 64], num_sector
 * outside [1, 256], num_candidates outside [1, 16], max_radius not finite or not > 0, lidar_height / search_ratio / dist_thres not finite (search_ratio < 0),
 * num_exclude_recent < 0, tree_period < 1, a frame outside the handle, n outside [1, 2^20], Q outside [1, 65536], P outside [1, 2^20], a node outside the
 * database, db_end outside [0, size], options whose num_ring / num_sector differ from the database's. iba_last_error(h) carries the message of
 * iba_sc_describe, iba_sc_last_error(db) of the calls on a database (db = NULL: of the calls that have neither, on this thread).
 * Limits: a node is a resident scan of a handle. A voxel-averaged cloud (the reference describes LoadPCD's output) becomes a node the way it becomes a
 * registration target: as a frame of the handle iba_submap_handle returns, without leaving the device. A database does not grow: describe
 * the whole run at once (Scan Context does not depend on poses) and bound each query with db_end. The PCL overload of makeScancontext and
 * detectLoopClosureIDBetweenSession are not restated (a query with an explicit db_end covers the latter's search). One GPU. The database has a stream of
 * its own and outlives the handle it was described from.
 */
#define IBA_SC_MAX_RING 64
#define IBA_SC_MAX_SECTOR 256
#define IBA_SC_MAX_CANDIDATES 16
#define IBA_SC_NO_WINNER 10000000.0
typedef struct iba_sc_options {
    int32_t struct_size;         /* sizeof(iba_sc_options) */
    int32_t num_ring;            /* PC_NUM_RING 20 */
    int32_t num_sector;          /* PC_NUM_SECTOR 60 */
    int32_t num_exclude_recent;  /* NUM_EXCLUDE_RECENT 30 (iba_sc_replay_plan) */
    int32_t num_candidates;      /* NUM_CANDIDATES_FROM_TREE 3 */
    int32_t tree_period;         /* TREE_MAKING_PERIOD_ 30 (iba_sc_replay_plan) */
    double  max_radius;          /* PC_MAX_RADIUS 80 */
    double  lidar_height;        /* LIDAR_HEIGHT 0 */
    double  search_ratio;        /* SEARCH_RATIO 0.1 */
    double  dist_thres;          /* SC_DIST_THRES 0.2 */
} iba_sc_options;
typedef struct iba_sc_query {
    int32_t struct_size;         /* sizeof(iba_sc_query) */
    int32_t node;                /* the descriptor that asks */
    int32_t db_end;              /* it is searched against the nodes [0, db_end); 0: no search (an early-returned call) */
    int32_t reserved;            /* 0 */
} iba_sc_query;
typedef struct iba_sc_result {
    int32_t struct_size;         /* written by the library: sizeof(iba_sc_result) */
    int32_t loop_node;           /* -1: none */
    int32_t shift;               /* of the winning candidate (0 when none won) */
    int32_t n_candidates;        /* min(num_candidates, db_end) */
    double  min_dist;            /* IBA_SC_NO_WINNER when no candidate won */
    float   yaw_rad;
    int32_t reserved;
    int32_t cand_node[IBA_SC_MAX_CANDIDATES];   /* in search order; -1 beyond n_candidates */
    int32_t cand_shift[IBA_SC_MAX_CANDIDATES];  /* -1 beyond n_candidates */
    double  cand_dist[IBA_SC_MAX_CANDIDATES];   /* NaN beyond n_candidates */
} iba_sc_result;
typedef struct iba_sc_db iba_sc_db;
/* the reference's constants (Scancontext.h) */
iba_status iba_default_sc_options(iba_sc_options* opt);
/* Descriptors, ring keys, sector keys and column norms of n resident scans (local frames of the handle; a frame may repeat) as nodes 0 .. n - 1 of a
 * database on the device: one launch chain (bins by integer atomic max, finalise + keys) and one synchronise. *out is NULL on failure. */
iba_status iba_sc_describe(iba_handle* h, const int32_t* frames, int32_t n, const iba_sc_options* opt, iba_sc_db** out);
int32_t iba_sc_db_size(const iba_sc_db* db);   /* nodes; 0 for NULL */
/* Copies of nodes [first, first + count) to the host; every output may be NULL. desc: count x num_ring x num_sector doubles, row-major [ring][sector];
 * ring_key: count x num_ring doubles; ring_key_f: their float narrowing (what the search reads); sector_key: count x num_sector doubles; n_skipped: the
 * points of the node's scan with a non-finite coordinate. */
iba_status iba_sc_db_read(iba_sc_db* db, int32_t first, int32_t count, double* desc, double* ring_key, float* ring_key_f, double* sector_key, int64_t* n_skipped);
void iba_sc_db_free(iba_sc_db* db);
const char* iba_sc_last_error(const iba_sc_db* db);   /* never NULL */
/* distanceBtnScanContext(node pairs[p][0], node pairs[p][1]) for P pairs in one launch: rule 5 */
iba_status iba_sc_distance(iba_sc_db* db, const int32_t* pairs /* P x 2 */, int32_t P, const iba_sc_options* opt, double* dist /* P */, int32_t* shift /* P */);
/* Q queries in one launch chain (search, distances of every (query, candidate), pick) and one synchronise: rules 6 and 7 */
iba_status iba_sc_detect(iba_sc_db* db, const iba_sc_query* queries, int32_t Q, const iba_sc_options* opt, iba_sc_result* out /* Q */);
/* Host only, no device: detectLoopClosureID's statefulness as a pure function. sizes_at_call[i] = the descriptors the manager holds at its i-th call (the
 * query of that call is node sizes_at_call[i] - 1). With fewer than num_exclude_recent + 1 descriptors the call returns early WITHOUT advancing the
 * counter: db_end[i] = 0. Otherwise, when counter % tree_period == 0 the search set becomes the first size - num_exclude_recent keys, then the counter
 * advances; between rebuilds the set is stale. db_end[i] = the size of the set call i searches. */
iba_status iba_sc_replay_plan(const int32_t* sizes_at_call, int32_t n, const iba_sc_options* opt, int32_t* db_end /* n */);

/*
 * ---- F-LOAM feature extraction: the edge cloud and the surf cloud of every scan [src/floam/src/laserProcessingClass.cpp: featureExtraction :12-98,
 * featureExtractionFromSector :101-211; called once per scan from System::Track] ----
 * The first half of the reference's LiDAR front end splits every raw scan into edge points (the sharpest of each sector of each laser ring) and surf
 * points (the rest); everything after it (updatePointsToMap, the edge and surf factors, the local map) reads only those two clouds. It depends on the
 * scan alone, never on a pose: here a BATCH OF RESIDENT SCANS (local frames of a handle, a frame may repeat; a scans-only handle is enough) is split in
 * one launch chain, and the two clouds of every scan come back in an object the library allocates, as iba_submap_build's do.
 *
 * Rules, fixed here so that the result is a function of the input alone (tests/floam_ref.py restates them in numpy; the device result equals it byte
 * for byte, indices and coordinates). Every operation below is rounded on its own: NO fused multiply-add; sqrt and / are IEEE. No floating-point atomics.
 *   1 point      the scan's float32 coordinates in the scan's ORIGINAL index order (the handle stores a scan in kd-leaf order; the original order is
 *                recovered on the device). A point with a non-finite coordinate is skipped and counted (n_nonfinite). d = sqrt(x x + y y) in f64 on
 *                the widened coordinates; a point with d < min_distance || d > max_distance is skipped and counted (n_out_of_range); angle =
 *                atan(z / d) * 180 / pi in f64. Known deviation: the reference forms x x + y y in float.
 *   2 ring       the reference's three expressions with C truncation towards zero. 16 lines: int((angle + 15) / 2 + 0.5). 32 lines: int((angle +
 *                92.0 / 3.0) * 3.0 / 4.0). 64 lines: int((2 - angle) * 3.0 + 0.5) when angle >= -8.83, else 32 + int((-8.83 - angle) * 2.0 + 0.5), and
 *                the point is skipped when angle > 2 || angle < -24.33. For every line count the point is skipped when the id is outside [0, num_lines)
 *                (or the angle is NaN: d == 0 with min_distance <= 0). These points are counted in n_no_ring. d is IEEE and reproduces to the bit; the
 *                f64 atan of two correct libraries may differ by an ulp, which matters only for a point whose angle sits on a boundary of these
 *                expressions (the tests keep their inputs 0.01 degrees away from every boundary).
 *   3 ring list  the points of a ring in original index order (a stable partition). A ring with fewer than min_ring_points points gives nothing; one
 *                with more than IBA_FLOAM_MAX_RING_POINTS answers IBA_ERR_UNSUPPORTED with a message naming the scan and the ring.
 *   4 curvature  for the positions j in [5, n - 5) of a ring of n points, per axis IN FLOAT32 and left to right as the reference writes it:
 *                ((((p[j-5] + p[j-4]) + p[j-3]) + p[j-2]) + p[j-1]) - 10 p[j] + p[j+1] + p[j+2] + p[j+3] + p[j+4] + p[j+5], the product rounded before
 *                the subtraction; value = (dx dx + dy dy) + dz dz in f64 on the widened differences; a NaN value counts as +inf. neighbour_span = 5 is
 *                the only supported window (any other value: IBA_ERR_INVALID_ARG).
 *   5 sectors    the reference's off-by-one is kept: with total = n - 10 and len = total / num_sectors (integer division), sector s holds the
 *                curvature entries [len s, end), end = len (s + 1) - 1 for s < num_sectors - 1 and total - 1 for the last sector. The last entry of
 *                every sector belongs to no sector and appears in neither cloud. A sector with no entries gives nothing.
 *   6 order      a sector's entries ascending by (value, position). Known deviation: std::sort leaves the order of equal values unspecified; here
 *                the lower position comes first.
 *   7 edges      the entries are walked in DESCENDING order with a picked set that starts empty per sector. For each entry whose position is not
 *                picked: stop when value <= edge_curvature; count it and mark it; when the count exceeds max_edges_per_sector stop (that entry stays
 *                marked and is in neither cloud); otherwise it is an edge point, and for k = 1 .. 5 upwards and, separately, k = -1 .. -5 downwards
 *                position ind + k is marked, a direction stopping at the first consecutive pair whose squared gap exceeds neighbour_gap2 (per-axis
 *                differences in float32, squared and summed in f64 as (dx dx + dy dy) + dz dz, strict '>'). A mark outside the sector has no effect.
 *   8 surf       the entries in ASCENDING order of rule 6 whose position is not marked.
 *   9 output     rings ascending, sectors ascending; within a sector the edges in pick order and the surfs in rule-8 order. *_xyz are the scan's own
 *                float32 values, untouched; *_index is the original index in the scan. A scan's result does not depend on what else is in the batch,
 *                and two calls give the same bytes.
 * Answers IBA_ERR_INVALID_ARG with a message, before any launch: a NULL argument, a struct_size of another library, num_lines not 16, 32 or 64, n outside
 * [1, 2^20], a frame outside the handle, distances not finite or min_distance > max_distance, min_ring_points < 11, num_sectors outside [1, 64],
 * max_edges_per_sector outside [0, 64], neighbour_span != 5, thresholds not finite. On failure *out is NULL and iba_last_error(h) carries the message.
 * Limits: iba_floam_extract brings the clouds back to the host; to register against them yourself, build a handle from them with iba_create.
 * iba_floam_odom_run (below) keeps them on the device as frames of a handle it builds there. The ring of a point is always derived from its elevation (a per-point
 * ring field supplied by the caller is not read). The scan-to-map step that consumes the clouds is iba_floam_map_* (below); PCL's VoxelGrid and crop
 * box are iba_lattice_build and the local map is kept by iba_floam_odom_run. One GPU.
 */
#define IBA_FLOAM_MAX_RING_POINTS 8192
typedef struct iba_floam_options {
    int32_t struct_size;          /* sizeof(iba_floam_options) */
    int32_t num_lines;            /* 16, 32 or 64 (lidar.h num_lines); default 64 */
    double  min_distance;         /* 3.0 (floamClass.cpp, HDL_64) */
    double  max_distance;         /* 90.0 (floamClass.h) */
    int32_t min_ring_points;      /* 131 */
    int32_t num_sectors;          /* 6 */
    int32_t max_edges_per_sector; /* 20 */
    int32_t neighbour_span;       /* 5 */
    double  edge_curvature;       /* 0.1 */
    double  neighbour_gap2;       /* 0.05 */
} iba_floam_options;
typedef struct iba_floam_features iba_floam_features;
/* the reference's constants */
iba_status iba_default_floam_options(iba_floam_options* opt);
/* The edge and surf clouds of n resident scans (local frames of the handle; a frame may repeat) as scans 0 .. n - 1 of the result: one launch chain
 * (classify, stable partition by (scan, ring), one block per sector, gather). The result is allocated by the library; release it with iba_floam_free. */
iba_status iba_floam_extract(iba_handle* h, const int32_t* frames, int32_t n, const iba_floam_options* opt, iba_floam_features** out);
/* Scans in the result (0 for NULL); edge / surf points of scan s (-1 for NULL or s out of range); their coordinates (3 floats per point) and their
 * original indices in the scan (valid until iba_floam_free; NULL for NULL or s out of range). */
int32_t iba_floam_num(const iba_floam_features* f);
int64_t iba_floam_n_edge(const iba_floam_features* f, int32_t s);
int64_t iba_floam_n_surf(const iba_floam_features* f, int32_t s);
const float* iba_floam_edge_xyz(const iba_floam_features* f, int32_t s);
const int32_t* iba_floam_edge_index(const iba_floam_features* f, int32_t s);
const float* iba_floam_surf_xyz(const iba_floam_features* f, int32_t s);
const int32_t* iba_floam_surf_index(const iba_floam_features* f, int32_t s);
/* The skipped points of scan s by reason and the points of each of its num_lines rings (before rule 3); every output may be NULL. */
iba_status iba_floam_stats(const iba_floam_features* f, int32_t s, int64_t* n_nonfinite, int64_t* n_out_of_range, int64_t* n_no_ring, int32_t* ring_points /* num_lines */);
void iba_floam_free(iba_floam_features* f);

/*
 * ---- F-LOAM scan-to-map: edge / surf factors and registration against given map clouds [src/floam/src/odomEstimationClass.cpp: updatePointsToMap
 * :32-110, addEdgeCostFactor :132-170, addSurfCostFactor :172-208; src/floam/src/lidarOptimization.cpp: EdgeAnalyticCostFunction,
 * SurfNormAnalyticCostFunction, PoseSE3Parameterization::Plus, getTransformFromSe3] ----
 * The stage that turns the edge and surf clouds of a scan into a LiDAR pose: every edge point is matched to the line through its 5 nearest map edge
 * points, every surf point to the plane through its 5 nearest map surf points, and a robustified 6-parameter problem is solved for the pose, twice
 * (optimization_count) with a new association each time. Here a BATCH OF PAIRS (scan clouds, map clouds, start pose) is evaluated together; all four
 * clouds of a pair are local frames of one handle (a scans-only handle from iba_create is enough; a frame of iba_submap_handle's handle is a voxel
 * cloud). A frame may appear in any number of pairs. The association leaves its factor records on the device; an LM trial re-reads them.
 *
 * Rules, fixed here so that the result is a function of the input alone (tests/floam_map_ref.py restates them in numpy). Every f64 operation is rounded
 * on its own (no fused multiply-add) except the three fma rows of the query transform. Every sum runs in a fixed order, no floating-point atomics: two
 * calls give the same bytes and a pair's result does not depend on the rest of the batch.
 *   1 query       the source point's float32 coordinates widened to double, lp_r = fma(T[r][2], z, fma(T[r][1], y, fma(T[r][0], x, T[r][3]))) (the rows
 *                 of iba_icp_* / iba_scan_*). KNOWN DEVIATION: the query is not narrowed back to float; PCL's kd tree searches the float point.
 *   2 neighbours  the five map points of least d^2 = (dx dx + dy dy) + dz dz, f64 on the widened floats, ascending by (d^2, original index): ties go to the
 *                 lowest index (KNOWN DEVIATION: FLANN keeps the first visited). A point yields a factor only if the map frame holds at least 5 points
 *                 and the 5th d^2 < max_nn_dist2, strictly; only such a point has neighbours in nn_idx. If the map edge frame holds at most min_map_edge
 *                 points or the map surf frame at most min_map_surf, the pair has NO factor of either kind (the reference's > 10 && > 50).
 *   3 edge        c = ((((p0 + p1) + p2) + p3) + p4) / 5 per axis; C = sum over the neighbours in order of (p - c)(p - c)^T; eigenvalues l0 <= l1 <= l2
 *                 of C, u the unit eigenvector of l2; kept iff l2 > edge_eig_ratio l1; a = c + edge_half_len u, b = c - edge_half_len u. With
 *                 nu = (lp - a) x (lp - b), de = a - b: r = |nu| / |de|, g = (de x (nu / |nu|)) / |de| (g = 0 when |nu| = 0), J = [lp x g, g] — the
 *                 1x6 of EdgeAnalyticCostFunction, -(nu^T / |nu|) skew(de) [-skew(lp), I] / |de|. r and J do not change under u -> -u: no sign rule.
 *   4 surf        n0 = the least-squares solution of A n0 = -1, A the 5x3 matrix of the neighbours in order (Householder QR, as the reference's
 *                 colPivHouseholderQr up to pivoting); d = 1 / |n0|, n = n0 / |n0|; kept iff all of these are finite and |(n . p_j) + d| <=
 *                 plane_max_resid for the five neighbours. r = (n . lp) + d, J = [lp x n, n] = n^T [-skew(lp), I].
 *   5 kernel      Huber IRLS as elsewhere in this library: w = 1 for |r| <= huber_delta, else huber_delta / |r|; rho = r^2, else 2 huber_delta |r| -
 *                 huber_delta^2; H += (w J)^T J, b += (w J)^T r, chi^2 += rho. KNOWN DEVIATION: Ceres's corrector also uses rho''.
 *   6 moments     IBA_FLOAM_NMOM doubles per pair: [0] edge points that passed rule 2, [1] edge factors kept, [2] surf points that passed rule 2,
 *                 [3] surf factors kept, [4..24] H, upper triangle by rows, [25..30] b, [31] chi^2, [32] sum r^2 of the edge factors, [33] of the surf
 *                 factors. The order of iba_scan_step: one partial per 64 positions of the source cloud in kd-leaf order, a wave's lanes by DPP, the
 *                 partials of a cloud by position, then edge cloud + surf cloud.
 *   7 records     per pair the points of the edge cloud, then of the surf cloud, each in its ORIGINAL order: an iba_floam_record with kind 0 none / 1 edge /
 *                 2 surf and v = a, b, 0 or n, d, 0, 0, 0; and, in nn_idx, 5 original map indices (0xFFFFFFFF x 5 for a point that failed rule 2). Pair
 *                 after pair.
 *   8 register    outer_passes times: associate at the current T (rules 1-4), then up to inner_iterations LM iterations on the FROZEN records — r, J
 *                 and w are re-evaluated at each trial pose, the search is not repeated. LM is the trust-region loop of csrc/iba_lm.hpp (its
 *                 LmOptions defaults; restated from Ceres's published algorithm, NOT Ceres) on 6 parameters, cost = chi^2 / 2: Jacobi scaling
 *                 1 / (1 + sqrt(H_ii)) fixed per pass; (Hs + clamp(diag Hs, 1e-6, 1e32) / radius) ds = -gs by the 6x6 LDL^T of the scan-to-scan
 *                 update; a trial pose T' = Exp(delta) T with delta = scale ds = [omega, upsilon] (the reference's Plus: the quaternion of
 *                 getTransformFromSe3, translation J(omega) upsilon, the small-angle branch below 1e-10 rad); gradient tolerance 1e-10 at the top
 *                 of an iteration, parameter tolerance 1e-8 against sqrt(1 + |t|^2) and function tolerance 1e-6 after the trial's evaluation,
 *                 acceptance at a relative decrease above 1e-3, radius /= max(1/3, 1 - (2 rho - 1)^3) or halved, quartered, .. on rejection; the
 *                 radius starts at 1e4 in every pass (the reference builds a new problem). A step whose model decrease is not positive shrinks
 *                 the radius without an evaluation. A pair ends IBA_FLOAM_MAP_DEGENERATE with its last valid T when a map is too small (rule 2),
 *                 an association keeps fewer than 6 factors, or a pivot is not positive and finite. The pairs of a batch advance together, one
 *                 launch chain and one synchronise per evaluation for all pairs still running.
 * Answers IBA_ERR_INVALID_ARG with a message in iba_last_error(h), before any launch: a NULL argument, a struct_size of another library, k != 5, a frame
 * outside the handle, a non-finite T, a threshold that is not finite or negative, a negative count, B outside [1, 4096].
 * Limits: the map clouds of these two calls are GIVEN (iba_submap_handle builds voxel clouds on the device); the loop that keeps a local map —
 * addPointsToMap with PCL's VoxelGrid and CropBox — is iba_floam_odom_run (below). laserMappingClass is not restated. A map cloud is always ONE frame and a frame of this library is one kd tree (one tile): the
 * search walks a single tree, its only box test is the frame's box against max_nn_dist2, and no bound is carried from tile to tile; a map spread over
 * several frames has to be merged into one first. The constant-velocity prediction of the start pose is the caller's here (iba_floam_odom_run forms it). Parity with Ceres and PCL is
 * unpinned (neither can be built beside this library). One GPU.
 */
#define IBA_FLOAM_NMOM 34
#define IBA_FLOAM_MAP_OK 0
#define IBA_FLOAM_MAP_DEGENERATE 1
typedef struct iba_floam_pair {             /* one registration problem */
    int32_t src_edge_frame, src_surf_frame; /* the scan's edge / surf cloud */
    int32_t map_edge_frame, map_surf_frame; /* the map's edge / surf cloud */
    double  T[16];                          /* row-major 4x4, scan frame -> map frame */
} iba_floam_pair;
typedef struct iba_floam_map_options {
    int32_t struct_size;          /* sizeof(iba_floam_map_options) */
    int32_t k;                    /* 5, the only supported neighbour count */
    double  max_nn_dist2;         /* 1.0 */
    double  edge_eig_ratio;       /* 3.0 */
    double  edge_half_len;        /* 0.1 */
    double  plane_max_resid;      /* 0.2 */
    double  huber_delta;          /* 0.1 */
    int32_t outer_passes;         /* 2: the reference's steady-state optimization_count (12 after initMapWithPoints) */
    int32_t inner_iterations;     /* 4 */
    int32_t min_map_edge;         /* 10 */
    int32_t min_map_surf;         /* 50 */
} iba_floam_map_options;
typedef struct iba_floam_record {
    int32_t kind;                 /* 0 none, 1 edge, 2 surf */
    int32_t tried;                /* 1: the point passed rule 2 */
    double  v[7];                 /* edge: a, b, 0; surf: n, d, 0, 0, 0 */
} iba_floam_record;
typedef struct iba_floam_map_result {
    double  T[16];                /* the final pose (the start pose for a pair that never ran) */
    double  initial_cost, final_cost;   /* chi^2 / 2 at the first association, after the last accepted step */
    int32_t passes, iterations, evaluations;
    int32_t n_edge, n_surf;       /* factors kept by the last association */
    int32_t status;               /* IBA_FLOAM_MAP_OK / IBA_FLOAM_MAP_DEGENERATE */
} iba_floam_map_result;
/* the reference's constants */
iba_status iba_default_floam_map_options(iba_floam_map_options* opt);
/* One association and evaluation per pair at pairs[b].T: search, fit, sums. nn_idx: NULL, or 5 entries per source point; records: NULL, or one per
 * source point (rule 7: sum over the pairs of P(src_edge_frame) + P(src_surf_frame) points). */
iba_status iba_floam_map_step(iba_handle* h, const iba_floam_pair* pairs, int32_t B, const iba_floam_map_options* opt,
                              double* moments /* B x IBA_FLOAM_NMOM */, uint32_t* nn_idx, iba_floam_record* records);
/* Rule 8 per pair from pairs[b].T, all pairs together. */
iba_status iba_floam_map_register(iba_handle* h, const iba_floam_pair* pairs, int32_t B, const iba_floam_map_options* opt, iba_floam_map_result* out /* B */);

/*
 * ---- F-LOAM odometry: local map upkeep and the track loop [src/floam/src/floamClass.cpp System::Track; src/floam/src/odomEstimationClass.cpp:
 * initMapWithPoints :25-29, updatePointsToMap :32-81, downSamplingToMap :94-99, addPointsToMap :210-250] ----
 * The loop that joins iba_floam_extract and iba_floam_map_register into what the reference's floam_kitti produces: a pose per scan. A BATCH OF
 * TRACKS (lists of resident scans of one handle) goes in, a pose per scan comes out, and nothing of cloud size crosses PCIe in between: the
 * feature clouds, the down-sampled clouds and the local maps become frames of handles that are built on the device (csrc/iba_index_kernels.hpp).
 * Rules, per track (tests/floam_odom_ref.py restates the filter and the host-side rules in numpy):
 *   O1 features     iba_floam_extract's rules on every scan of every track: ONE chain for the whole call (it depends on no pose).
 *   O2 down-sample  downSamplingToMap: the lattice filter (iba_lattice_build, rules L1-L4) without crop on each scan's clouds in the scan's own
 *                   frame, edge cloud leaf = map_resolution, surf cloud leaf = 2 map_resolution, centroids narrowed to float32 (round to nearest
 *                   even): ONE chain for the whole call.
 *   O3 first scan   initMapWithPoints: pose T0; the map is the RAW, un-down-sampled edge and surf features moved by T0 (rule L1's expression,
 *                   narrowed to float32), no crop, no filter. The step record has passes = 0 and T_pred = T = T0.
 *   O4 prediction   for k >= 1, T_pred = T[k-1] (inv(T[k-2]) T[k-1]) with T[-1] := T0; inv = [R^T, -R^T t]; f64 on the host.
 *   O5 solve        rule 8 of iba_floam_map_* from T_pred on (down-sampled scan clouds, map of step k - 1) with max(map.outer_passes,
 *                   init_passes - k) passes: the reference's optimization_count, 12 after init, one less on every scan, down to 2. A DEGENERATE
 *                   pair keeps the pose the solve returns (the reference keeps its prediction when the map is too small) and the track goes on.
 *   O6 map update   addPointsToMap, per kind: members [map of step k - 1, identity; down-sampled scan cloud, T[k]], crop t[k] +- crop_half per axis
 *                   (f64), the lattice filter with leaf map_resolution (edge) / 2 map_resolution (surf), narrowed to float32. Map points therefore
 *                   stay in (ix, iy, iz) order, old map first within a cell.
 *   O7 batch        the tracks of a call advance in lock-step: one extract chain, one down-sampling chain, then per step one solve and one map
 *                   update for all tracks still running. Tracks may differ in length and a frame may appear in several tracks. A track's result
 *                   does not depend on the rest of the batch, and two calls give the same bytes.
 * Answers IBA_ERR_INVALID_ARG with a message, before any launch: a NULL argument, B outside [1, 256], n_scans outside [1, 2^16], a frame outside
 * the handle, a non-finite T0, map_resolution or crop_half not positive and finite, init_passes < 0, a wrong struct_size (nested ones included);
 * the checks of the two nested option blocks run too and are reported under this function's name. IBA_ERR_UNSUPPORTED: more than 2048 scans in
 * one call (the down-sampling chain takes two sub-maps per scan), a cloud of 2^22 points or more, a map that spans more than 2^17 cells along an
 * axis, a coordinate that is not finite after narrowing to float32.
 * Limits: a first version — every step builds a small handle (the four clouds of every running track) on the device and releases the one
 * before; csrc/iba_floam_odom_host.hpp and DESIGN.md say what a step allocates. laserMappingClass (the global map for display) is not restated.
 * Parity with Ceres and PCL is unpinned, as for iba_floam_map_*. One GPU.
 */
typedef struct iba_floam_track {
    int32_t n_scans;
    const int32_t* frames;        /* [n_scans] local frames of the handle, in time order */
    double  T0[16];               /* row-major 4x4, the pose of the first scan */
} iba_floam_track;
typedef struct iba_floam_odom_options {
    int32_t struct_size;          /* sizeof(iba_floam_odom_options) */
    int32_t init_passes;          /* 12 */
    int32_t keep_maps;            /* 0; 1: the map after every step stays readable (tests) */
    int32_t reserved;             /* 0 */
    double  map_resolution;       /* 0.4 (HDL_64; 0.2 for 16 / 32 lines) */
    double  crop_half;            /* 100.0 */
    iba_floam_options     extract;
    iba_floam_map_options map;    /* outer_passes is the floor of the pass count (2) */
} iba_floam_odom_options;
typedef struct iba_floam_odom_step {
    double  T_pred[16], T[16];
    double  initial_cost, final_cost;
    int32_t passes, iterations, evaluations, n_edge, n_surf, status;
    int64_t n_src_edge, n_src_surf;   /* the down-sampled scan clouds */
    int64_t n_map_edge, n_map_surf;   /* the map AFTER this step */
} iba_floam_odom_step;
typedef struct iba_floam_odom iba_floam_odom;
/* the reference's constants, the nested blocks included */
iba_status iba_default_floam_odom_options(iba_floam_odom_options* opt);
/* B tracks in lock-step. The result is allocated by the library; release it with iba_floam_odom_free. *out is NULL on failure. */
iba_status iba_floam_odom_run(iba_handle* h, const iba_floam_track* tracks, int32_t B, const iba_floam_odom_options* opt, iba_floam_odom** out);
/* Tracks of a result (0 for NULL); scans of track b (-1 out of range); its n_scans step records (NULL out of range); the down-sampled cloud of
 * scan k and the map after step k (kind 0 edge / 1 surf; 3 floats per point, *n points; the map of the last step always, of any step with
 * keep_maps; NULL with *n = -1 otherwise). Valid until iba_floam_odom_free. */
int32_t iba_floam_odom_num(const iba_floam_odom* o);
int32_t iba_floam_odom_n_scans(const iba_floam_odom* o, int32_t b);
const iba_floam_odom_step* iba_floam_odom_steps(const iba_floam_odom* o, int32_t b);
const float* iba_floam_odom_src(const iba_floam_odom* o, int32_t b, int32_t k, int32_t kind, int64_t* n);
const float* iba_floam_odom_map(const iba_floam_odom* o, int32_t b, int32_t k, int32_t kind, int64_t* n);
void iba_floam_odom_free(iba_floam_odom* o);

/*
 * ---- Pose-graph optimisation: Levenberg-Marquardt with line process [backend_opt.cpp:433-528 MultiRegistration: nodes pose[i]^-1 :441, odometry
 * edges (i-1, i) :454 / :472, loop edges (uncertain) :507, GlobalOptimization(PoseGraph, GlobalOptimizationLevenbergMarquardt(), criteria,
 * GlobalOptimizationOption(MRmaxCorrDist, MREdgePruneThre, 1.0, 0)) :515-525] ----
 * The last step of the reference's LiDAR back end: the edges and 6x6 informations that leave iba_scan_register become a pose graph, LM runs on it,
 * uncertain edges whose line-process weight stayed below edge_prune_threshold are dropped, and LM runs again on what is left. Open3D solves every LM
 * trial with a dense 6N x 6N ldlt(); here the graph is what it is in that back end — a chain with a few cross edges — and a trial is a block
 * arrowhead elimination on the device (below). An iba_pgo is a stand-alone object on one device (no iba_handle needed); everything of size N or E stays
 * on the device between LM trials, the host reads a handful of scalars per trial.
 *
 * Restated from Open3D's public GlobalOptimization sources AS REMEMBERED (Open3D is not part of the reference tree: parity with it is UNPINNED).
 * WHERE THIS RESTATEMENT AND OPEN3D DIFFER, THIS TEXT IS THE CONTRACT: tests/pgo_ref.py restates it in numpy and the tests hold the device to that.
 * Transforms are row-major 4x4 with the last row 0 0 0 1; a rigid inverse is always formed as [R^T, -R^T t]; all arithmetic is IEEE f64.
 *   1 vec6           v = [a, b, c, tx, ty, tz] of a transform M: sy = sqrt(M00^2 + M10^2); sy >= 1e-6: a = atan2(M21, M22), b = atan2(-M20, sy),
 *                    c = atan2(M10, M00); otherwise a = atan2(-M12, M11), b = atan2(-M20, sy), c = 0. Its inverse T(v) = Rz(c) Ry(b) Rx(a) with the
 *                    translation (the map of the point-to-plane update of iba_scan_*).
 *   2 misalignment   of edge (s, t, X, L): M = X^-1 pose_t^-1 pose_s, zeta = vec6(M).
 *   3 Jacobian       column k of Js = lin6(X^-1 pose_t^-1 G_k pose_s), lin6(M) = [(M21 - M12) / 2, (M02 - M20) / 2, (M10 - M01) / 2, M03, M13, M23]; G_0..2 the
 *                    so(3) generators about x, y, z (as 4x4), G_3..5 the unit translations. Jt = -Js exactly, so an edge has ONE block A = w Js^T L Js
 *                    and one vector g = w Js^T L zeta: H_ss += A, H_tt += A, H_st = H_ts -= A, b_s -= g, b_t += g. Only the upper triangle of L
 *                    (info) is read; it is mirrored.
 *   4 line process   mu = preference_loop_closure * max_corr_dist^2 * (mean of L(5,5) over the uncertain edges of the graph being solved, in edge order),
 *                    0 without one. An uncertain edge: w = (mu / (mu + zeta^T L zeta))^2 (mu + zeta^T L zeta == 0: w = 1); a certain edge: w = 1. Weights start
 *                    at 1 and are recomputed after every ACCEPTED step, at the accepted poses, before the system is rebuilt.
 *   5 residual       r = sum over the edges of w zeta^T L zeta with the weights in force (a trial's r_new: the trial poses, the weights of the last
 *                    linearisation; after an accepted step r is the residual of the relinearisation, i.e. with the NEW weights).
 *   6 LM             linearise; lambda = 1e-5 * (largest diagonal entry of H), nu = 2. An OUTER ITERATION: (a) max |b| < min_right_term stops
 *                    IBA_PGO_STOP_RIGHT_TERM; (e) after max_iteration outer iterations IBA_PGO_STOP_MAX_ITERATION; then up to max_iteration_lm TRIALS:
 *                    delta = (H + lambda I)^-1 b; (b) |delta| < min_relative_increment * (|x| + min_relative_increment), x the stacked vec6 of the
 *                    poses, stops IBA_PGO_STOP_INCREMENT (the trial counts, nothing is applied); trial pose_i = T(delta_i) pose_i; rho = (r - r_new) /
 *                    (delta . (lambda delta + b) + 1e-3). rho > 0: lambda *= max(lower_scale_factor, min(1 - (2 rho - 1)^3, upper_scale_factor)), nu = 2,
 *                    the step is accepted (weights, relinearisation), (c) r_before - r_new < min_relative_residual_increment * r_before stops
 *                    IBA_PGO_STOP_RESIDUAL_INCREMENT, and the outer iteration ends. Otherwise lambda *= nu, nu *= 2, next trial. An outer iteration
 *                    whose trials are all rejected ends as it is. After an outer iteration (d) r < min_residual stops IBA_PGO_STOP_RESIDUAL.
 *                    Checks in the order a, e, b, c, d as the loop meets them. The system is NOT gauge-fixed: lambda I makes it definite (lambda = 0 or a
 *                    pivot that is not positive and finite: IBA_ERR_UNSUPPORTED). After a pass, with reference_node >= 0, every pose is left-multiplied by
 *                    pose_ref(before the pass) * pose_ref(after)^-1.
 *   7 pruning        after pass 1 an uncertain edge with w < edge_prune_threshold is dropped; pass 2 runs on what is left from pass 1's poses, weights
 *                    reset to 1, mu recomputed, lambda and nu started anew.
 * The linear solve (iba_pgo_solve, every trial): a CHAIN EDGE is the first edge, in edge order, between nodes i and i + 1 in either direction; every
 * other edge is a CROSS EDGE. The separator set S = the endpoints of all cross edges and every node i with i % K == 0; K = segment, doubled until
 * |S| <= IBA_PGO_MAX_SEPARATORS (cross-edge endpoints alone beyond the cap: IBA_ERR_INVALID_ARG naming the count). The maximal runs of
 * non-separator nodes are block tridiagonal and independent: forward block LDL^T of D + lambda I along each run, its Schur complement added to the
 * run's two bounding separators, in run order; the 6|S| x 6|S| separator system by a blocked right-looking Cholesky and two triangular solves; back
 * substitution along the runs. No floating-point atomics, every sum in a fixed order: two calls give the same bytes. iba_pgo_plan (host only) answers
 * the separators and runs for a graph. Memory: O((N + E) 36 + |S|^2 36) doubles.
 * Answers IBA_ERR_INVALID_ARG with a message, BEFORE the device is probed: a NULL argument, struct_size, N < 1, E < 0, a source / target outside [0, N)
 * or source == target, a number that is not finite (poses, T, the upper triangle of info, the options), a pose or T whose last row is not exactly
 * 0 0 0 1, reference_node outside [-1, N), segment < 1, max_iteration / max_iteration_lm < 0. iba_pgo_last_error(pg) carries the message of a call
 * on pg; iba_pgo_last_error(NULL) of the calls without one (create, plan), on this thread.
 * Limits: one GPU; a graph whose cross edges touch more than IBA_PGO_MAX_SEPARATORS nodes. The incremental path (UpdateISAM) is iba_smooth_* (below).
 */
#define IBA_PGO_MAX_SEPARATORS 1024
#define IBA_PGO_STOP_NONE 0               /* the pass did not run */
#define IBA_PGO_STOP_RIGHT_TERM 1
#define IBA_PGO_STOP_INCREMENT 2
#define IBA_PGO_STOP_RESIDUAL_INCREMENT 3
#define IBA_PGO_STOP_RESIDUAL 4
#define IBA_PGO_STOP_MAX_ITERATION 5
typedef struct iba_pgo_edge { int32_t source, target; double T[16]; double info[36]; int32_t uncertain; } iba_pgo_edge; /* PoseGraphEdge: T row-major 4x4, info row-major 6x6 [rotation, translation] as iba_scan_result.info */
typedef struct iba_pgo_options {
    int32_t struct_size;               /* sizeof(iba_pgo_options) */
    int32_t reference_node;            /* 0; -1: no compensation */
    double  max_corr_dist;             /* backend.yml MRmaxCorrDist 1.2 */
    double  edge_prune_threshold;      /* MREdgePruneThre 0.25 */
    double  preference_loop_closure;   /* 1.0 */
    int32_t max_iteration;             /* MRmaxIter 100 */
    int32_t max_iteration_lm;          /* 20 */
    double  min_relative_increment, min_relative_residual_increment, min_right_term, min_residual;   /* 1e-6 each */
    double  upper_scale_factor, lower_scale_factor;   /* 2/3, 1/3 */
    int32_t segment;                   /* separator spacing K; 128, the fastest of 8 .. 128 in profiles/pgo_bench.md */
    int32_t reserved;                  /* 0 */
} iba_pgo_options;
typedef struct iba_pgo_pass { int32_t iterations, trials, stop, reserved; double residual, lambda; } iba_pgo_pass;   /* outer iterations, LM trials, IBA_PGO_STOP_*, final r and lambda */
typedef struct iba_pgo_result {
    int32_t struct_size;               /* written by the library: sizeof(iba_pgo_result) */
    int32_t n_pruned;                  /* uncertain edges dropped after pass 1 */
    iba_pgo_pass pass[2];
} iba_pgo_result;
typedef struct iba_pgo iba_pgo;
iba_status iba_default_pgo_options(iba_pgo_options* opt);
/* nodes16: N row-major 4x4 poses (the reference passes pose[i]^-1). The graph is copied; *out is NULL on failure. */
iba_status iba_pgo_create(const double* nodes16, int32_t N, const iba_pgo_edge* edges, int32_t E, const iba_pgo_options* opt, int device, iba_pgo** out);
void iba_pgo_destroy(iba_pgo* pg);
const char* iba_pgo_last_error(const iba_pgo* pg);   /* never NULL */
/* Host only, no device: the separators (ascending; up to sep_cap written, *n_separators their number), the runs as (first, last) node pairs in
 * ascending order (up to run_cap pairs written, *n_runs their number) and the K actually used. Every output may be NULL. Pose values are not needed:
 * of an edge only source and target are read. */
iba_status iba_pgo_plan(int32_t N, const iba_pgo_edge* edges, int32_t E, const iba_pgo_options* opt, int32_t* separators, int32_t sep_cap, int32_t* n_separators,
                        int32_t* runs /* 2 per run */, int32_t run_cap, int32_t* n_runs, int32_t* K_used);
/* Linearises at the current poses with the weights in force (rules 2, 3, 5; a dropped edge has A = 0 and adds nothing). Every output may be NULL:
 * zeta E x 6, weight E, A E x 36 (row-major, w Js^T L Js), b N x 6, *residual. */
iba_status iba_pgo_linearize(iba_pgo* pg, double* zeta, double* weight, double* A, double* b, double* residual);
/* (H + lambda I) delta = b at the last linearisation (IBA_ERR_STATE without one); delta N x 6 */
iba_status iba_pgo_solve(iba_pgo* pg, double lambda, double* delta);
/* The whole GlobalOptimization: rules 6 and 7 */
iba_status iba_pgo_optimize(iba_pgo* pg, iba_pgo_result* result);
/* The state: poses N x 16, weights E, dropped flags E bytes. Every output may be NULL. */
iba_status iba_pgo_read(iba_pgo* pg, double* nodes16, double* weight, uint8_t* pruned);

/*
 * ---- Robust smoothing of a chain-with-loops pose graph [backend_opt.cpp:242-431 LoopClosureRun / LoopClosureRegThread / UpdateISAM: the noise
 * models :108-113 (Cauchy::Create(1) over the loop variances), PriorFactor :198-200, the odometry BetweenFactor prevPose.between(currPose) :206, a robust
 * BetweenFactor per verified loop :266, isam->update() and calculateBestEstimate() :375-381] ----
 * The smoothing stage of the reference's LiDAR back end, the one that yields floam_isam_xx.txt. An iba_smooth is a stand-alone object on one device
 * (no iba_handle needed) whose graph GROWS: nodes and factors are appended between updates, iba_smooth_update optimises every node present from the
 * current estimates. Everything of size N or F stays on the device between LM trials.
 *
 * KNOWN DEVIATIONS (GTSAM is not part of the reference tree: parity with it is UNPINNED, as for iba_pgo_* and iba_scan_*):
 *   - iSAM2's incremental Bayes-tree algorithm (a few Gauss-Newton steps of the affected cliques per update()) is NOT restated. iba_smooth_update
 *     runs Levenberg-Marquardt to the CONVERGED robust optimum of the same factor graph over all nodes.
 * THIS TEXT IS THE CONTRACT: tests/smooth_ref.py restates it in numpy and the tests hold the device to that. Transforms are row-major 4x4 with the
 * last row 0 0 0 1; a rigid inverse is always formed as [R^T, -R^T t]; all arithmetic is IEEE f64 without contraction; no floating-point atomics,
 * every sum in a fixed order: two calls give the same bytes.
 *   S1 poses, tangents  P_i maps body to world (FramePoses, gtsam::Pose3). xi = [omega, upsilon], rotation first (GTSAM's order). Exp(xi) = [R, t]:
 *                    R = I + a W + b W^2, t = (I + b W + c W^2) upsilon, W = [omega]x, theta = |omega|, a = sin(theta) / theta, b = (1 - cos(theta)) /
 *                    theta^2, c = (theta - sin(theta)) / theta^3. Log([R, t]): the quaternion (w, v) of R by its largest component, w >= 0,
 *                    omega = (2 atan2(|v|, w) / |v|) v — exact up to theta = pi — and upsilon = (I - W / 2 + e W^2) t, e = (1 - (theta / 2)
 *                    cot(theta / 2)) / theta^2. SERIES: with theta^2 < 1e-2 each of a, b, c, e (and c2, k4 of S2) is its Taylor polynomial in theta^2
 *                    through theta^10 (c2, k4: theta^8); with (|v| / w)^2 < 2.5e-3 the factor 2 atan2(|v|, w) / |v| is (2 / w) (1 - u / 3 + u^2 / 5 -
 *                    u^3 / 7 + u^4 / 9 - u^5 / 11), u = (|v| / w)^2. r = 0 exactly (every odometry factor and the prior start there) is the normal case.
 *   S2 residual      a prior (j, Z): r = Log(Z^-1 P_j); a between factor (i, j, Z): r = Log(Z^-1 P_i^-1 P_j). Perturbations on the left, in the world
 *                    frame: P <- Exp(delta) P. J = dr / d delta_j = Jr^-1(r) Ad(P_j^-1); for a between factor dr / d delta_i = -J exactly.
 *                    Ad([R, t]) = [[R, 0], [[t]x R, R]]. Jr^-1(r) = [[Ji, 0], [-Ji Q Ji, Ji]], Ji = I + W / 2 + e W^2 and, with U = [upsilon]x,
 *                    d = omega . upsilon: Q = -U / 2 + c (W U + U W + d W) - c2 (W W U + U W W + 3 d W) - 2 k4 d W W (Barfoot's Q block at -r),
 *                    c2 = (theta^2 / 2 + cos(theta) - 1) / theta^4, k4 = (c2 + 3 (c - 1/6) / theta^2) / 2. So a factor has ONE block
 *                    A = w J^T S^-1 J and one vector g = w J^T S^-1 r, S = diag(var): a between factor H_ii += A, H_jj += A, H_ij = H_ji -= A,
 *                    b_i += g, b_j -= g; a prior H_jj += A, b_j -= g.
 *   S3 robust weight q = sum r_k^2 / var_k. A robust factor (Cauchy, k = 1): w = 1 / (1 + q), and it adds log1p(q) to F; any other factor w = 1 and
 *                    adds q. F is twice the loss. Weights are recomputed at every linearisation.
 *   S4 LM            rule 6 of iba_pgo_* with F in the place of r (a trial's F_new is F at the trial poses), the same option fields and stops
 *                    (IBA_PGO_STOP_*; x of stop (b) the stacked vec6 of rule 1 there), the trial pose Exp(delta_i) P_i, and lambda_0 = 1e-5 * the
 *                    largest diagonal entry of the BETWEEN-factor part of H (the priors are left out: at the reference's prior variance 1e-12 they
 *                    would put lambda seven orders above the odometry information). One pass: no pruning, no reference-node compensation.
 *   S5 solve         the block-arrowhead chain of iba_pgo_* (chain factor: the first between factor, in call order, on nodes i and i + 1; separators,
 *                    runs, blocked Cholesky), the same kernels. The plan is rebuilt on the host whenever nodes or factors were added since the
 *                    last one. Cross factors touching more than IBA_PGO_MAX_SEPARATORS nodes: IBA_ERR_INVALID_ARG from the call that plans.
 * Answers IBA_ERR_INVALID_ARG with a message, BEFORE the device is touched: a NULL argument, struct_size, a number that is not finite, a pose or Z whose
 * last row is not exactly 0 0 0 1, a node outside the graph or i == j, a variance that is not finite or not > 0, segment < 1, max_iteration /
 * max_iteration_lm < 0, first / count outside the graph. iba_smooth_last_error(s) carries the message of a call on s; iba_smooth_last_error(NULL)
 * that of iba_smooth_create, on this thread. A graph without a node: IBA_ERR_STATE from linearize / solve / update.
 * A device failure while the graph is brought onto the device loses the estimates: the call answers IBA_ERR_HIP, every later one IBA_ERR_STATE.
 * Limits: one GPU; factors cannot be removed; Gaussian or Cauchy(1) noise on a diagonal covariance only. LONG TRAJECTORIES: stop (b) compares |delta|
 * with 1e-6 of the stacked pose vector, and lambda_0 follows the largest diagonal entry of H, whose rotation part carries |t|^2 / var lever arms of
 * world-frame perturbations. On a trajectory of hundreds of metres (500 nodes and more in profiles/backend_bench.md) the first trial's step falls under
 * that stop at the default options and iba_smooth_update applies nothing; convergence is shown at N <= 130. Lower min_relative_increment there.
 */
typedef struct iba_smooth_options {
    int32_t struct_size;               /* sizeof(iba_smooth_options) */
    int32_t max_iteration;             /* 100 */
    int32_t max_iteration_lm;          /* 20 */
    int32_t segment;                   /* separator spacing K of the solve, 128 */
    double  min_relative_increment, min_relative_residual_increment, min_right_term, min_residual;   /* 1e-6 each */
    double  upper_scale_factor, lower_scale_factor;   /* 2/3, 1/3 */
} iba_smooth_options;
typedef struct iba_smooth_result {
    int32_t struct_size;               /* written by the library: sizeof(iba_smooth_result) */
    int32_t n_nodes, n_factors;        /* the graph that was optimised */
    int32_t iterations, trials, stop;  /* outer iterations, LM trials, IBA_PGO_STOP_* */
    double  F_start, F, lambda_start, lambda, max_b;   /* F and lambda before and after; max |b| at the final poses */
} iba_smooth_result;
typedef struct iba_smooth iba_smooth;
iba_status iba_default_smooth_options(iba_smooth_options* opt);
iba_status iba_smooth_create(const iba_smooth_options* opt, int device, iba_smooth** out);   /* *out is NULL on failure */
void iba_smooth_destroy(iba_smooth* s);
const char* iba_smooth_last_error(const iba_smooth* s);   /* never NULL */
/* Appends node n (0, 1, 2 ... in call order) with pose16 as its estimate. */
iba_status iba_smooth_add_node(iba_smooth* s, const double* pose16);
/* Factors are numbered 0, 1, 2 ... in call order, priors and between factors together. var6: the diagonal of S in [omega, upsilon] order. */
iba_status iba_smooth_add_prior(iba_smooth* s, int32_t node, const double* Z16, const double* var6);
iba_status iba_smooth_add_between(iba_smooth* s, int32_t i, int32_t j, const double* Z16, const double* var6, int32_t robust);
/* Linearises at the current estimates (S2, S3). Every output may be NULL: r F x 6, w F, A F x 36 (row-major), D N x 36 (the diagonal blocks of H),
 * b N x 6, *F. */
iba_status iba_smooth_linearize(iba_smooth* s, double* r, double* w, double* A, double* D, double* b, double* F);
/* (H + lambda I) delta = b at the last linearisation (IBA_ERR_STATE without one, or when the graph grew since); delta N x 6 */
iba_status iba_smooth_solve(iba_smooth* s, double lambda, double* delta);
/* S4 over every node present, from the current estimates */
iba_status iba_smooth_update(iba_smooth* s, iba_smooth_result* result);
/* The estimates of nodes first .. first + count - 1 (count x 16) and the weights of ALL factors at the last linearisation (F doubles; 1 before any).
 * Either output may be NULL. */
iba_status iba_smooth_read(iba_smooth* s, int32_t first, int32_t count, double* nodes16, double* weight);

/*
 * ---- The back end's loop-closure run: options and plan [backend_opt.cpp:322-370 SCManage, :304-314 PerformLoopClosure; config/loam/backend.yml,
 * BackEndOption backend_opt.h:48-85] ----
 * iba_backend_plan (host only, no device) is SCManage's bookkeeping as a pure function of the raw poses: which frames become keyframes, which
 * frame's cloud is described for each, which keyframes call detectLoopClosureID, and the sizes_at_call sequence iba_sc_replay_plan takes. With it
 * the run is a composition of what is above: iba_submap_handle over the described frames -> iba_sc_describe -> iba_sc_replay_plan + iba_sc_detect
 * (Scan Context never depends on the optimised poses) -> per detection iba_submap_build / iba_scan_register -> iba_smooth_add_between +
 * iba_smooth_update. iba_backend_run is that composition as one call on a handle whose frames 0 .. N - 1 are the raw scans (scans only is enough):
 *   1 the plan; 2 the voxel clouds of all described frames as ONE iba_submap_handle batch; 3 one iba_sc_describe; 4 the whole detection sequence as one
 *   iba_sc_detect; 5 a prior on node 0 at the raw pose; 6 per frame j the factor between(raw_(j-1), raw_j) = raw_(j-1)^-1 raw_j at odom_var and node j
 *   at its raw pose; 7 at a detection with loop node k, history = keyframes[k]: the sub-map over frames [max(0, history - S), min(history + S, N)),
 *   S = lc_submap_size, posed by the CURRENT poses (estimates for nodes already optimised, raw for the others), brought into the history frame by
 *   out12 = pose[history]^-1 (formed as [R^T, -R^T t], as every rigid inverse of this library), is the target frame and the query keyframe's voxel cloud the source frame of a two-frame iba_submap_handle, and
 *   iba_scan_register (opt->scan) runs from the identity; 8 the loop is accepted iff fitness > loop_overlap_thre && inlier_rmse <
 *   loop_inlier_rmse_thre, both strict; 9 on accept between(history, j, T, loop_var, robust), iba_smooth_update, and the estimates of nodes 0 .. j
 *   become the current poses; 10 after the last frame one more update.
 * KNOWN DEVIATION: a loop is verified at the moment it is detected, with the poses current then; in the reference the timing of the loop-closure
 * thread decides which poses a sub-map sees. The detection records hold every loop Scan Context found (accepted or not) in frame order. Errors of the
 * composed calls come back with this function's name in front (iba_backend_last_error). Nothing of cloud size crosses PCIe. The smoother runs on the
 * handle's device (iba_handle_device).
 * Rules (poses12: N row-major 3x4, the KITTI layout; frame 0 is keyframe 0, describes itself and is never a query). For j = 1 .. N - 1:
 * PoseDif(pose_(j-1), pose_j) = (|t_j - t_(j-1)|, the angle of R = R_j R_(j-1)^T taken as atan2(s, c), c = (trace(R) - 1) / 2, s = half the norm of
 * (R21 - R12, R02 - R20, R10 - R01)) is added to four accumulators (sequential f64 sums). translation > keyframe_meter_gap || rotation >
 * keyframe_rad_gap (both strict): both reset, j becomes a keyframe and describes frame j - cloud_lag; THEN, and only then, the loop-closure pair is
 * tested against lc_keyframe_meter_gap / lc_keyframe_rad_gap (strict): both reset and the keyframe is a query, sizes_at_call = the keyframes so far.
 * IBA_ERR_INVALID_ARG with a message (iba_backend_last_error, per thread): a NULL opt or poses12, struct_size, N < 1, a number that is not finite,
 * a variance not > 0, voxel not > 0, lc_submap_size < 0, cloud_lag or keep_update_poses other than 0 or 1.
 */
typedef struct iba_backend_options {
    int32_t struct_size;               /* sizeof(iba_backend_options) */
    int32_t lc_submap_size;            /* LCSubmapSize 25 */
    double  voxel;                     /* odom.voxel 0.2 */
    double  keyframe_meter_gap, keyframe_rad_gap;         /* 1.5, 0.15 */
    double  lc_keyframe_meter_gap, lc_keyframe_rad_gap;   /* 3, 1 */
    double  loop_overlap_thre, loop_inlier_rmse_thre;     /* 0.5, 0.2: a loop is accepted iff fitness > and inlier_rmse <, both strict (:263) */
    iba_sc_options sc;                 /* iba_default_sc_options; dist_thres = scDistThres 0.2, max_radius = scMaximumRadius 80 (backend_opt.h:60-61) */
    iba_scan_options scan;             /* the loop registration as written (:262): point-to-point, coarse 1.0 m x 1 iteration (1e-4), refine
                                          0.3 m x 0 iterations (1e-6), no information matrix */
    double  prior_var[6], odom_var[6], loop_var[6];       /* backend_opt.h:81-83: 1e-12; 1e-6 x 3, 1e-4 x 3; 0.5 */
    iba_smooth_options smooth;         /* iba_default_smooth_options */
    int32_t cloud_lag;                 /* 1: a keyframe j describes LoadPCD(j - 1), as :360 does; 0: its own scan */
    int32_t keep_update_poses;         /* 0; 1: the result keeps the estimates after every update (iba_backend_result_update_poses12), n_nodes x 12 doubles each */
} iba_backend_options;
iba_status iba_default_backend_options(iba_backend_options* opt);
const char* iba_backend_last_error(void);   /* never NULL; of this thread's last iba_backend_* call that failed */
/* Every output may be NULL; keyframes, described, detects and sizes_at_call hold up to N entries. keyframes[k]: the frame of keyframe k (KeyFrameQuery);
 * described[k]: the frame whose cloud is node k of the Scan Context database; detects[k]: 1 when keyframe k is a query; sizes_at_call[c]: the
 * descriptors held at call c (its query is node sizes_at_call[c] - 1). */
iba_status iba_backend_plan(const double* poses12, int32_t N, const iba_backend_options* opt, int32_t* keyframes, int32_t* described, uint8_t* detects,
                            int32_t* n_keyframes, int32_t* sizes_at_call, int32_t* n_calls);
typedef struct iba_backend_detection {
    int32_t query_frame, history_frame, accepted, reserved;
    double  sc_dist, fitness, rmse;   /* Scan Context's min_dist; iba_scan_register's fitness and inlier_rmse */
    double  T[16];                    /* row-major 4x4, query cloud -> history frame: the loop factor's measurement */
} iba_backend_detection;
typedef struct iba_backend_result iba_backend_result;
/* *out is NULL on failure; release it with iba_backend_result_free. */
iba_status iba_backend_run(iba_handle* h, const double* poses12, int32_t N, const iba_backend_options* opt, iba_backend_result** out);
void iba_backend_result_free(iba_backend_result* r);
/* Of a result (0 / NULL for NULL), valid until it is freed: the N final poses, 12 doubles per row in the KITTI layout writePoses writes; the keyframes;
 * the detections; the iba_smooth_result of every update (one per accepted loop, then the final one). */
int32_t iba_backend_result_n_frames(const iba_backend_result* r);
const double* iba_backend_result_poses12(const iba_backend_result* r);
int32_t iba_backend_result_n_keyframes(const iba_backend_result* r);
const int32_t* iba_backend_result_keyframes(const iba_backend_result* r);
int32_t iba_backend_result_n_detections(const iba_backend_result* r);
const iba_backend_detection* iba_backend_result_detections(const iba_backend_result* r);
int32_t iba_backend_result_n_updates(const iba_backend_result* r);
const iba_smooth_result* iba_backend_result_updates(const iba_backend_result* r);
/* With opt->keep_update_poses: the estimates after update u, updates[u].n_nodes rows of 12 doubles (the current poses of nodes 0 .. n_nodes - 1 that the
 * next sub-map is posed by); NULL without the option or for u out of range. */
const double* iba_backend_result_update_poses12(const iba_backend_result* r, int32_t u);

/*
 * ---- Scan-to-image projection: z-buffered depth, visibility, colours [what a caller does with a calibrated extrinsic: the README pictures
 * doc/proj_XX_gt.png / proj_XX_pred.png of the reference, a sparse depth image per camera frame, a colour per LiDAR point] ----
 * A JOB is one (local frame of the handle, extrinsic x) pair; the J jobs of a call may repeat frames, so one frame can be rendered under the initial,
 * the ground-truth and the optimised extrinsic. Everything is computed on the device and stays there until an accessor copies one job's product down.
 * All arithmetic is IEEE f64 without contraction, all reductions are integer (minima and counts): no floating-point atomics, two calls give the same
 * bytes, and tests/project_ref.py restates every rule in numpy and is compared byte for byte.
 *
 *   P1 pose.       R, t = Sim3Exp(x) on the host (csrc/iba_host_math.hpp), as the evaluator forms them. The scale entry x[6] does not enter: it scales
 *                  camera translations, not LiDAR points. The 12 doubles (R | t, row-major 3 x 4) are kept per job: iba_projection_pose.
 *   P2 transform.  The point's float32 coordinates are widened; q_k = ((R_k0 x + R_k1 y) + R_k2 z) + t_k. A point with a non-finite coordinate is
 *                  skipped and counted (n_skipped).
 *   P3 projection. IN_FRONT iff z_min < q_z < z_max, both strict. u = (fx q_x + cx q_z) / q_z, v = (f q_y + cy q_z) / q_z with f = fy, or fx under
 *                  v_focal_is_fx (the evaluator's rule, iba_global.cpp:73). The quotients come from the evaluator's device helper (div2,
 *                  csrc/iba_kernels.hpp), which tests/test_gpu_division.py pins as equal to plain division. INSIDE iff 0 <= u < W && 0 <= v < H. The
 *                  pixel is (iu, iv) = (floor(u), floor(v)). The depth is z32 = q_z rounded to float32.
 *   P4 z-buffer.   key = (bits of z32) << 32 | original point index — the point's position in the caller's scan, not its kd-leaf position. z32 is
 *                  not negative, so keys order like depths and a tie goes to the lowest index. Every INSIDE point lowers, by a 64-bit integer atomic
 *                  min, the key of every pixel of its footprint [iu - r, iu + r] x [iv - r, iv + r] clipped to the image (r = splat). Empty = all ones.
 *   P5 images.     Depth = the winning key's z32, 0 for an empty pixel; index = its point, 0xFFFFFFFF for an empty pixel (row-major H x W).
 *                  n_pixels = the pixels that hold a key.
 *   P6 visibility. An INSIDE point is VISIBLE iff (double)z32 <= (double)zwin * (1.0 + occlusion_tol), zwin the depth of the final key at the point's
 *                  own centre pixel (a point is always inside its own footprint, so zwin exists).
 *   P7 colour.     For a VISIBLE point: bilinear at (u, v), pixel centres at integer coordinates. x0 = floor(u), x1 = min(x0 + 1, W - 1), a = u - x0,
 *                  likewise y0, y1, b from v. Per channel c = ((1 - a) * ((1 - b) * c00 + b * c01)) + (a * ((1 - b) * c10 + b * c11)), the first
 *                  index of c being x; the byte is floor(c + 0.5). A point that is not VISIBLE gets 0 0 0.
 *   P8 overlay.    The output is the input image, or black for NULL; a pixel that holds a key takes iba_project_gradient(zn),
 *                  zn = min(max((z - z_near) / (z_far - z_near), 0), 1), z the pixel's depth widened. The gradient is this five-stop piecewise-linear
 *                  ramp: zn = 0 blue (0, 0, 255), 0.25 cyan (0, 255, 255), 0.5 green (0, 255, 0), 0.75 yellow (255, 255, 0), 1 red (255, 0, 0);
 *                  s = 4 zn, k = min(floor(s), 3), f = s - k, c = (1 - f) * stop_k + f * stop_(k+1) per channel, the byte floor(c + 0.5).
 *                  iba_project_gradient clamps zn to [0, 1] itself (NaN: 0).
 *   P9 counts.     All counts are integers, so every reduction order gives the same value.
 *
 * A point's record (iba_projection_points): flags = IN_FRONT 1 | INSIDE 2 | VISIBLE 4; (u, v) and z32 are as computed for an IN_FRONT point and 0
 * otherwise (skipped points included).
 * MEMORY: the result keeps 8 bytes per pixel (depth, index) and 24 bytes per point of every job. The z-buffer's keys (8 bytes per pixel) live only
 * while a CHUNK of consecutive jobs runs: the jobs of a call are cut so that a chunk's key, depth and index images (16 bytes per pixel and job) stay
 * under IBA_PROJECT_BUDGET_BYTES, or under a quarter of the device memory free at the call where that is less; a chunk holds at least one job. A chunk
 * boundary changes no byte. The result does not depend on the handle once iba_project_run has returned.
 * ERRORS, all IBA_ERR_INVALID_ARG with a message (iba_project_last_error, per thread) BEFORE the device is touched: a NULL argument or a wrong
 * struct_size; J < 1 or a frame outside the handle's local frames; a non-finite x or option, splat outside 0..4, occlusion_tol < 0, not
 * 0 < z_min < z_max, not z_near < z_far, v_focal_is_fx not 0 / 1; a camera that is partly zero, not finite, with fx, fy <= 0 or W, H not whole, or
 * W H outside [1, 2^26]; a frame without intrinsics (every frame of a scans-only handle of iba_submap_handle) while camera is all 0 — the message names the
 * frame; a job index outside the result.
 */
#define IBA_PROJECT_BUDGET_BYTES (1ull << 30)
#define IBA_PROJECT_IN_FRONT 1u
#define IBA_PROJECT_INSIDE   2u
#define IBA_PROJECT_VISIBLE  4u
typedef struct iba_project_options {
    int32_t struct_size;     /* sizeof(iba_project_options) */
    int32_t splat;           /* 1: half-width r of the square footprint, 0..4 */
    double  occlusion_tol;   /* 0.02: relative depth slack of P6, finite and >= 0 */
    double  z_min, z_max;    /* 0.1, 120: depth range in metres, 0 < z_min < z_max */
    int32_t v_focal_is_fx;   /* 0; 1 reproduces the evaluator's rule for v (fx for both, iba_global.cpp:73) */
    int32_t reserved;
    double  camera[6];       /* fx, fy, cx, cy, W, H. All 0: the frame's intrinsics; otherwise it overrides them for every job */
    double  z_near, z_far;   /* 2, 60: range of the overlay's gradient */
} iba_project_options;
typedef struct iba_project_counts {
    int64_t n_points, n_skipped, n_in_front, n_inside, n_visible, n_pixels;
} iba_project_counts;
typedef struct iba_projection iba_projection;
iba_status iba_default_project_options(iba_project_options* opt);
const char* iba_project_last_error(void);   /* never NULL; of this thread's last iba_project_* / iba_projection_* call that failed */
/* x7: J x 7 (the evaluator's x), frames: J local frames. *out is NULL on failure; release it with iba_projection_free. The four kernels (splat,
 * resolve, visible, and per accessor colourise / overlay) are csrc/iba_project_kernels.hpp; the run launches on the handle's stream and synchronises once. */
iba_status iba_project_run(iba_handle* h, const double* x7, const int32_t* frames, int32_t J, const iba_project_options* opt, iba_projection** out);
void iba_projection_free(iba_projection* p);
int32_t iba_projection_n_jobs(const iba_projection* p);                                    /* 0 for NULL */
iba_status iba_projection_size(const iba_projection* p, int32_t job, int32_t* W, int32_t* H);
iba_status iba_projection_pose(const iba_projection* p, int32_t job, double Rt12[12]);     /* the R | t the device used (P1) */
iba_status iba_projection_counts(const iba_projection* p, int32_t job, iba_project_counts* counts);
iba_status iba_projection_depth(iba_projection* p, int32_t job, float* depth_HxW);
iba_status iba_projection_index(iba_projection* p, int32_t job, uint32_t* index_HxW);
/* per point in the ORIGINAL order of the frame's scan; any of the three may be NULL */
iba_status iba_projection_points(iba_projection* p, int32_t job, double* uv_nx2, float* z_n, uint8_t* flags_n);
iba_status iba_projection_colorize(iba_projection* p, int32_t job, const uint8_t* rgb_HxWx3, uint8_t* point_rgb_nx3);   /* P7: one launch */
iba_status iba_projection_overlay(iba_projection* p, int32_t job, const uint8_t* rgb_HxWx3 /* may be NULL: black */, uint8_t* out_HxWx3);   /* P8: one launch */
iba_status iba_project_gradient(double zn, uint8_t rgb[3]);                                /* host only: the overlay's palette */

/*
 * ---- ORB feature extraction: pyramid, FAST, oriented BRIEF [the camera side's first brick: ORBextractor::operator(), src/orb_slam/src/ORBextractor.cc
 * of the reference, for a batch of 8-bit images that may differ in size] ----
 * Nearly everything is per-pixel integer work; tests/orb_ref.py restates every rule in numpy and the device results are compared byte for byte. Unless
 * stated otherwise float arithmetic is float32, every operation rounded, no contraction; rint = round half to even (cvRound).
 *
 *   O1 levels.     sf[0] = 1, sf[l] = sf[l-1] * scale_factor, inv[l] = 1 / sf[l]; Wl = rint((float)W * inv[l]), Hl likewise; a level with Wl < 1 or
 *                  Hl < 1 is empty. Features per level as the constructor (:436-446): factor = 1 / scale_factor, d = n_features * (1 - factor) /
 *                  (1 - (float)pow((double)factor, (double)n_levels)); level l < L - 1 takes rint(d), then d *= factor; the last takes what is left, at
 *                  least 0. 2000 / 1.2 / 8 gives 434 362 302 251 209 175 145 122.
 *   O2 resize.     Level l from level l - 1. Per axis: scale = (double)src / dst; f = (float)((d + 0.5) * scale - 0.5); s = floor(f); f -= s; s < 0:
 *                  s = 0, f = 0; s >= src - 1: s = src - 1, f = 0; c1 = rint(f * 2048), c0 = 2048 - c1. The host builds these tables; the kernel is
 *                  integer: S = p[s] * c0 + p[s + 1] * c1 per source row (p[s + 1] is not read where s = src - 1: its weight is 0),
 *                  out = (((b0 * (S0 >> 4)) >> 16) + ((b1 * (S1 >> 4)) >> 16) + 2) >> 2. The reference's 19-pixel reflected border around a level is
 *                  not built: no output depends on it.
 *   O3 cells.      minB = 16, maxBX = Wl - 16, maxBY = Hl - 16, width = maxBX - minB, height likewise; nCols = floor(width / 30), nRows =
 *                  floor(height / 30); a level with nCols < 1 or nRows < 1 has no cells and no keypoints (the reference divides by zero there and
 *                  ends with none). wCell = ceil(width / nCols), hCell = ceil(height / nRows). Cell (i, j) is the sub-image [iniX, maxX) x [iniY, maxY)
 *                  of :789-806: iniX = minB + j wCell, maxX = min(iniX + wCell + 6, maxBX), likewise Y with i; FAST tests its pixels at distance >= 3
 *                  from the sub-image's border: [iniX + 3, maxX - 3) x [iniY + 3, maxY - 3). A cell exists iff that region is not empty (the
 *                  reference's skip tests drop exactly the empty columns, and FAST finds nothing in an empty row). The regions tile
 *                  [19, Wl - 19) x [19, Hl - 19) without overlap.
 *   O4 FAST score. The 16-pixel Bresenham circle of radius 3. Per polarity the arc value is the minimum over 9 consecutive circle pixels of v_k - p
 *                  (bright) or p - v_k (dark); score = the maximum over the 16 arcs and both polarities, minus 1: the largest t for which 9 contiguous
 *                  pixels are all > p + t or all < p - t. A pixel is a corner at t iff score >= t. One uint8 score map per level serves both
 *                  thresholds: 0 where score < min_th_fast and at pixels nearer than 3 to the level's edge.
 *   O5 per cell.   Among a cell's tested pixels with score >= ini_th_fast keep those whose score is strictly greater than all 8 neighbours'; a neighbour
 *                  counts as 0 outside the cell's tested region or below the threshold, so two equal adjacent corners remove each other. None kept:
 *                  repeat with min_th_fast and count a fallback cell. A level's candidates are ordered by cell (i, then j), inside a cell by row,
 *                  then column; coordinates are relative to minB (what the reference hands to DistributeOctTree); response = score.
 *   O6 distribution (host, iba_orb_distribute). DistributeOctTree and DivideNode (:481-763) restated exactly: n_ini = round(width / height) in float,
 *                  hX = width / n_ini, the start nodes with truncated corners, a candidate's start node (int)(x / hX); the two phases, the list order
 *                  (children pushed to the front, n1..n4), the stop tests, a result of >= N and up to N + 3 nodes (also for N = 0, as in the
 *                  reference), the best response per node with the first winning a tie. ONE RULE IS THE LIBRARY'S OWN: the reference sorts
 *                  (size, node address) pairs in its second phase, so equal sizes are ordered by heap address; here, among equal sizes, the node
 *                  created later is divided first.
 *   O7 orientation. Integer moments m10 = sum u I, m01 = sum v I over the 31-row circular patch at the keypoint's pixel in the UNBLURRED level, row v
 *                  spanning |u| <= umax[|v|], umax = 15 15 15 15 14 14 14 13 13 12 11 10 9 8 6 3 (the constructor's rule). angle = the degree
 *                  arctangent polynomial of ((float)m01, (float)m10): with ax = |x|, ay = |y|, c = min / (max + (float)DBL_EPSILON), c2 = c c,
 *                  a = (((p7 c2 + p5) c2 + p3) c2 + p1) c, p1 p3 p5 p7 = 0.9997878412794807f, -0.3258083974640975f, 0.1555786518463281f,
 *                  -0.04432655554792128f, each times (float)(180 / pi); ax < ay: a = 90 - a; x < 0: a = 180 - a; y < 0: a = 360 - a.
 *   O8 blur.       Every level that has keypoints: separable 7 taps, integer weights 18 34 49 54 49 34 18 (256 exp(-k^2 / 8) / sum rounded, the centre
 *                  taking the remainder), reflect-101 at the level's own border; horizontal sums are exact in 16 bits, vertical out =
 *                  (sum + 32768) >> 16. A level without keypoints is not blurred: its blurred stage reads as zeros.
 *   O9 descriptor. a_rad = angle * (float)(pi / 180); cos and sin of (double)a_rad from ONE fixed sequence of f64 operations (csrc/iba_orb_host.hpp,
 *                  orb_sincos: q = floor(x * 2/pi + 0.5), r = (x - q pio2_hi) - q pio2_lo, the sine and the cosine polynomial in Horner form, the
 *                  quadrant swap; the same function on host and device), each rounded to float: a = cos, b = sin. A pattern point (x, y) is read at
 *                  row = rint(x * b + y * a), col = rint(x * a - y * b) from the keypoint in the BLURRED level: two products and one sum each. Bit k of
 *                  byte i is t0 < t1 of test 8 i + k. Keypoints lie >= 19 pixels from the level's edge and pattern points within radius 18: no read
 *                  can leave the level and there is no clamp.
 *   O10 output.    Levels in ascending order, inside a level the order of O6's node list. xy = (level pixel, i.e. candidate + 16) * sf[l];
 *                  size = (int)(31 * sf[l]); octave = l; response = score; angle in degrees.
 *
 * KNOWN DEVIATIONS / UNPINNED. The library does not link OpenCV: five rules are its own integer restatements, modelled on
 * the reference's OpenCV calls and NOT pinned to recorded OpenCV outputs: O2 resize (cv::resize INTER_LINEAR), O8 blur (GaussianBlur 7 x 7, sigma 2),
 * O4 FAST score (cv::FAST's corner score), O5 the per-cell non-maximum suppression (cv::FAST with nonmaxSuppression), O7 the polynomial arctangent
 * (cv::fastAtan2). O6's tie rule is stated above. The BRIEF test-pair table is an INPUT (256 x 4 int8: x0 y0 x1 y1 per test); the library ships none.
 * Masks, undistortion and ComputeKeyPointsOld are not provided. Windowed matching is iba_orb_match below. Of the two vocabulary matchers,
 * SearchByBoW and SearchForTriangulation, the second is iba_triangulate further below with the DBoW2 node id of every keypoint as an INPUT (it needs
 * the outcome of the vocabulary, not the vocabulary); SearchByBoW remains unprovided, as do SearchBySim3 and the SearchByProjection overloads that take a
 * key frame (the overload that takes map points is iba_map_match further below). Two-view initialisation is iba_twoview_init further below; what Tracking::CreateInitialMapMonocular does after a success
 * (global BA, median-depth scaling) and the >= 100-matches gates around the call are the caller's.
 * DEVICE: one chain per chunk over flat tables (one row per image and level, per 64 x 16 tile, per cell, per keypoint): resize level by level, score,
 * cell count, scan, ordered cell write, the candidates down, O6 on the host, the keypoints up, orientation, blur, descriptor (csrc/iba_orb_kernels.hpp).
 * MEMORY: a chunk of consecutive images takes IBA_ORB_BYTES_PER_PIXEL bytes per pyramid pixel (pyramid, scores, blurred levels, the candidate
 * bound); a call is cut so that a chunk stays under IBA_ORB_BUDGET_BYTES, or under a quarter of the device memory free at the call where that is less; a
 * chunk holds at least one image and a chunk boundary changes no byte. Without keep_stages the planes live only for the call and the result is host
 * memory; with it the result owns pyramid, scores and blurred levels on the device (3 bytes per pyramid pixel) and the candidates on the host.
 * ERRORS, all IBA_ERR_INVALID_ARG with a message (iba_orb_last_error, per thread) BEFORE the device is touched: a NULL argument or a wrong struct_size;
 * n < 1; an image with W, H < 1 or stride < W; options outside the stated ranges, a scale_factor that is not finite or <= 1; pattern == NULL or a
 * pattern point outside the disc x^2 + y^2 <= 324; an image where some level has cells and n_ini == 0 (the reference would index out of bounds); an
 * image or level index outside the result; a stage accessor on a result without keep_stages.
 */
#define IBA_ORB_BUDGET_BYTES (1ull << 30)
#define IBA_ORB_BYTES_PER_PIXEL 6ull
typedef struct iba_orb_image   { const uint8_t* gray; int32_t W, H; int64_t stride; } iba_orb_image;   /* 8-bit, row-major, stride >= W bytes */
typedef struct iba_orb_options {
    int32_t struct_size;     /* sizeof(iba_orb_options) */
    int32_t n_features;      /* 2000, >= 1 */
    float   scale_factor;    /* 1.2f, finite and > 1 */
    int32_t n_levels;        /* 8, 1..16 */
    int32_t ini_th_fast;     /* 20 */
    int32_t min_th_fast;     /* 7, 1 <= min <= ini <= 254 */
    int32_t keep_stages;     /* 0; 1 keeps pyramid, score maps, candidates and blurred levels for the stage accessors */
    int32_t reserved;
    const int8_t* pattern;   /* 256 x 4: x0 y0 x1 y1 per test, every point with x*x + y*y <= 324; read during iba_orb_extract only */
} iba_orb_options;
typedef struct iba_orb_features iba_orb_features;
iba_status iba_default_orb_options(iba_orb_options* opt);            /* pattern = NULL: the caller must set it */
const char* iba_orb_last_error(void);                                /* never NULL; of this thread's last iba_orb_* call that failed */
/* *out is NULL on failure; release it with iba_orb_free */
iba_status iba_orb_extract(const iba_orb_image* images, int32_t n, const iba_orb_options* opt, int device, iba_orb_features** out);
void       iba_orb_free(iba_orb_features* f);
int32_t    iba_orb_n_images(const iba_orb_features* f);              /* 0 for NULL */
/* any output may be NULL; the three per-level arrays take n_levels entries */
iba_status iba_orb_counts(const iba_orb_features* f, int32_t image, int32_t* n_keypoints, int32_t* per_level, int32_t* candidates_per_level, int32_t* fallback_cells_per_level);
iba_status iba_orb_read(iba_orb_features* f, int32_t image, float* xy /* n x 2 */, float* angle, float* response, int32_t* octave, float* size, uint8_t* desc /* n x 32 */);   /* any may be NULL */
/* stage accessors, keep_stages only; a level's size is iba_orb_plan's */
iba_status iba_orb_level(iba_orb_features* f, int32_t image, int32_t level, int32_t blurred, uint8_t* out /* Hl x Wl */);
iba_status iba_orb_scores(iba_orb_features* f, int32_t image, int32_t level, uint8_t* out /* Hl x Wl, 0 = no corner */);
iba_status iba_orb_candidates(iba_orb_features* f, int32_t image, int32_t level, int32_t* xy /* n x 2, relative to minB */, int32_t* score);   /* n = candidates_per_level[level] */
/* host only, pure functions (precedents: iba_pgo_plan, iba_backend_plan). iba_orb_plan ignores opt->pattern; every output may be NULL; level_wh is
 * 0 0 for an empty level, cells 0 0 0 0 and n_ini 0 for a level without cells. */
iba_status iba_orb_plan(int32_t W, int32_t H, const iba_orb_options* opt, int32_t* level_wh /* L x 2 */, int32_t* features_per_level, int32_t* cells /* L x 4: nCols nRows wCell hCell */, int32_t* n_ini /* L */, int32_t umax[16]);
/* O6 on n candidates (0 <= x < width, 0 <= y < height): chosen receives *n_chosen <= n candidate indices in the order of the node list */
iba_status iba_orb_distribute(const int32_t* xy, const int32_t* score, int32_t n, int32_t width, int32_t height, int32_t N, int32_t* chosen /* cap n */, int32_t* n_chosen);

/*
 * ---- Windowed ORB descriptor matching [the camera side's second brick: the two call sites of the reference's ORBmatcher that need no vocabulary and
 * no map, SearchForInitialization (src/orb_slam/src/ORBmatcher.cc:405-520) and SearchByProjection(Frame&, const Frame&, th, bMono) (:1328-1470), on
 * Frame::AssignFeaturesToGrid, PosInGrid and GetFeaturesInArea (src/orb_slam/src/Frame.cc:230-245, :327-392)] ----
 * A call takes F frames and J jobs; a job matches the queries it lists against the keypoints of one frame (its train frame) under one of two rules.
 * All consecutive pairs of a sequence are one call. The work is integer work (cell indices, list order, popcounts, comparisons); tests/orb_match_ref.py
 * restates every rule in numpy and the device results are compared byte for byte. Float arithmetic is float32, every operation rounded, evaluated left
 * to right, no contraction; round = half away from zero (the C function the reference calls).
 *
 *   M1 frame.      n keypoints, each with xy (float32, the undistorted position), octave (int32), angle (float32 degrees), desc (32 bytes), and the four
 *                  float32 bounds min_x, max_x, min_y, max_y (the reference's mnMinX ..). The grid is 64 columns by 48 rows;
 *                  inv_w = 64.0f / (max_x - min_x), inv_h = 48.0f / (max_y - min_y).
 *   M2 grid.       (PosInGrid, AssignFeaturesToGrid) px = (int)round((x - min_x) * inv_w), py likewise with min_y and inv_h. A keypoint with px outside
 *                  [0, 64) or py outside [0, 48) is in no cell. It is round, not floor: the reference's rule, kept. A cell's list holds its keypoints
 *                  in ascending index. (The comparison with the range is made on the rounded float, so no product is too large to convert.)
 *   M3 area query. (GetFeaturesInArea(u, v, r, minLevel, maxLevel)) c0x = max(0, (int)floor((u - min_x - r) * inv_w)); c0x >= 64: the list is empty.
 *                  c1x = min(63, (int)ceil((u - min_x + r) * inv_w)); c1x < 0: empty. The same for y with 48 and 47. check = minLevel > 0 ||
 *                  maxLevel >= 0. Walk ix outer, iy inner, then the cell's list in its order; with check skip a keypoint whose octave < minLevel and,
 *                  where maxLevel >= 0, one whose octave > maxLevel; keep the keypoint iff fabs(x - u) < r && fabs(y - v) < r, both strict. The
 *                  list's order is part of the result: it decides ties.
 *   M4 distance.   The number of set bits of the XOR of the two 32-byte descriptors.
 *   M5 a query.    (u, v, r, minLevel, maxLevel, desc, angle, valid); desc and angle are those of keypoint query_index of the job's query frame. A
 *                  query that is not valid is never looked at and stays unmatched.
 *   M6 rule INIT.  (SearchForInitialization's loop, :418-487) Per train keypoint held_dist = INT_MAX and holder = -1. The queries in ascending index:
 *                  walk the list, skipping a candidate c with held_dist[c] <= dist; over the rest best = the least distance, held by the FIRST
 *                  candidate in list order that attains it (strict <); best2 = the second smallest value of the multiset (two candidates at the
 *                  same least distance give best2 == best; fewer than two candidates: INT_MAX). Accept iff best <= th_low and
 *                  (float)best < (float)best2 * nn_ratio. On accept: a candidate that has a holder takes that holder's match away (match[holder] =
 *                  -1, n_matches--, n_displaced++); then match[q] = c, holder[c] = q, held_dist[c] = best, n_matches++, and the QUERY is entered
 *                  into the rotation histogram (M8) with rot = angle_q - angle_c. A holder displaced later STAYS in the histogram's counts.
 *   M7 rule CLAIM. (the loop of :1351-1445 for the monocular case) Per train keypoint a claimed bit. The queries in ascending index: skip claimed
 *                  candidates; best starts at 256 and the first candidate with the strictly least distance wins (a candidate at distance 256 never
 *                  does); accept iff a candidate was found and best <= th_high. On accept: claim the candidate, match[q] = c, n_matches++, and the
 *                  TRAIN index is entered into the histogram with rot = angle_q - angle_c. As a claimed keypoint is claimed once, the entry names
 *                  the query as well. KNOWN DEVIATION: the reference skips a candidate only if its map point also has Observations() > 0; here every
 *                  claim counts.
 *   M8 rotation.   (check_orientation != 0) rot < 0.0f: rot += 360.0f. bin = (int)round(rot * (1.0f / 30)); bin == 30 becomes 0. The factor is the
 *                  reference's 1.0f / HISTO_LENGTH where 360.0f / HISTO_LENGTH would spread the bins, so the bins in use are 0..12: restated, not
 *                  corrected. ComputeThreeMaxima (:1601-1642) exactly: strict > in bin order (a count above max1 moves 1 to 2 and 2 to 3, one above
 *                  max2 moves 2 to 3); ind2 and ind3 are dropped when (float)max2 < 0.1f * (float)max1, else ind3 when (float)max3 < 0.1f *
 *                  (float)max1. Every entry of a bin other than the three loses its match: INIT decrements n_matches only where the entry still
 *                  holds a match, CLAIM always decrements (its entries all hold one). Without check_orientation hist is zeros and ind is -1 -1 -1.
 *   M9 outputs per job. match[n_queries] (the train index or -1), dist[n_queries] (the accepted distance of a surviving match, else -1), n_matches,
 *                  n_candidates (the sum of the list lengths), n_displaced (INIT), n_rot_removed (matches M8 took away), hist[30] (the counts at
 *                  push time), ind[3].
 *
 * THE TWO QUERY BUILDERS (host only, pure) restate what the reference's call sites hand to GetFeaturesInArea:
 *   iba_orb_match_init_queries: one query per keypoint of frame1, query_index = its index, valid iff octave == 0 (the reference skips level1 > 0; an
 *                  octave below 0 is not valid either), centre = prev_matched_xy, r = (float)window_size, levels (0, 0).
 *   iba_orb_match_motion_queries: (:1359-1390 for bMono) one query per keypoint i of the last frame; not valid where has_point[i] == 0 or outlier[i] != 0.
 *                  xc = ((R00 X + R01 Y) + R02 Z) + t0, yc and zc likewise with rows 1 and 2 of the current frame's Tcw (3 x 4 row-major, float32);
 *                  invzc = (float)(1.0 / (double)zc); not valid iff invzc < 0; u = fx * xc * invzc + cx, v = fy * yc * invzc + cy; not valid where
 *                  u < min_x, u > max_x, v < min_y or v > max_y of the CURRENT frame's bounds (a centre exactly on a bound is kept), and - the
 *                  library's own rule - where u or v is not finite; r = th * scale_factors[octave], levels (octave - 1, octave + 1). A query that is
 *                  not valid gets centre 0 0, radius 0 and levels 0 0. UNPINNED: the reference forms Rcw * X + tcw with OpenCV's 3 x 3 float product,
 *                  which may sum in another order than the one stated here.
 *
 * DEVICE (csrc/iba_orb_match_kernels.hpp): every frame goes up once, however many jobs name it. Grid: one thread per keypoint of any frame takes its
 * cell and counts per (frame, cell); a scan; one wave per frame fills the lists in ascending index by ballot-free lane ranks (no order depends on atomic
 * arrival). Lists: one thread per query counts its M3 list, the counts are scanned, and a second pass writes the candidate indices in M3's order
 * together with their M4 distances (one uint16 each). Resolve: ONE wave per job walks the queries in order; the lanes stride over the query's
 * segment, the wave combines (distance, list position) lexicographically and the second order statistic, lane 0 applies M6 or M7; the per-train
 * state is in LDS up to IBA_ORB_MATCH_LDS_TRAIN train keypoints and in global memory above; M8 runs at the end of the same kernel. The resolve is
 * sequential by the rule's definition: the parallelism is across jobs.
 * MEMORY: the frames, the queries and the grid of the whole call stay on the device for the call (60 bytes per keypoint, 36 per query, 8 per grid cell; a chunk adds 13 bytes per query of its jobs). The candidate
 * lists (IBA_ORB_MATCH_BYTES_PER_CANDIDATE bytes per entry, sized from the count pass) are cut into chunks of consecutive jobs under
 * IBA_ORB_MATCH_BUDGET_BYTES, or under a quarter of the device memory free at the call where that is less; a chunk holds at least one job and a chunk
 * boundary changes no byte. A chunk whose lists hold 2^31 entries or more answers IBA_ERR_UNSUPPORTED. The result is host memory.
 * ERRORS, all IBA_ERR_INVALID_ARG with a message (iba_orb_match_last_error, per thread) BEFORE the device is touched: a NULL argument (a frame's
 * arrays may be NULL only where n == 0, a job's where n_queries == 0; valid may always be NULL: all valid) or a wrong struct_size; F < 1, J < 1; a
 * frame with n < 0 or n > IBA_ORB_MATCH_MAX_KEYPOINTS; bounds that are not finite or max <= min; a keypoint position that is not finite; an angle
 * that is not finite or outside [0, 360] (the histogram's bins would leave the table); a job's frame or a query's query_index out of range; an unknown
 * rule; n_queries < 0; a centre or radius that is not finite, r < 0, or a magnitude above 1e6 (the reference's (int) of such a float is undefined);
 * nn_ratio not finite or <= 0; th_low or th_high outside [0, 256]; a job or frame index outside the result; a stage accessor on a result without
 * keep_stages. A frame with n == 0 and a job with n_queries == 0 are legal.
 */
#define IBA_ORB_MATCH_BUDGET_BYTES (1ull << 30)
#define IBA_ORB_MATCH_BYTES_PER_CANDIDATE 6ull
#define IBA_ORB_MATCH_MAX_KEYPOINTS 32768
#define IBA_ORB_MATCH_LDS_TRAIN 8192
#define IBA_ORB_MATCH_GRID_COLS 64
#define IBA_ORB_MATCH_GRID_ROWS 48
#define IBA_ORB_MATCH_HISTO 30
typedef enum iba_orb_match_rule { IBA_ORB_MATCH_INIT = 0, IBA_ORB_MATCH_CLAIM = 1 } iba_orb_match_rule;
typedef struct iba_orb_frame {                /* host pointers, read during the call only */
    const float*   xy;        /* n x 2 */
    const int32_t* octave;    /* n */
    const float*   angle;     /* n, degrees in [0, 360] */
    const uint8_t* desc;      /* n x 32 */
    int32_t n;
    float min_x, max_x, min_y, max_y;
} iba_orb_frame;
typedef struct iba_orb_match_job {
    int32_t query_frame, train_frame;   /* indices into the call's frame array; they may be equal */
    int32_t rule;                       /* iba_orb_match_rule */
    int32_t n_queries;
    const float*   centre_xy;           /* n_queries x 2 */
    const float*   radius;              /* n_queries */
    const int32_t* level_range;         /* n_queries x 2: minLevel maxLevel */
    const int32_t* query_index;         /* n_queries: the keypoint of query_frame that supplies descriptor and angle */
    const uint8_t* valid;               /* n_queries, or NULL: all valid */
} iba_orb_match_job;
typedef struct iba_orb_match_options {
    int32_t struct_size;        /* sizeof(iba_orb_match_options) */
    int32_t th_low;             /* 50: INIT's bound on best */
    int32_t th_high;            /* 100: CLAIM's bound on best */
    float   nn_ratio;           /* 0.9f: INIT's ratio */
    int32_t check_orientation;  /* 1 */
    int32_t keep_stages;        /* 0; 1 keeps the grid and the candidate lists for the stage accessors */
} iba_orb_match_options;
typedef struct iba_orb_match_counts {
    int32_t n_queries, n_matches, n_candidates, n_displaced, n_rot_removed;
    int32_t hist[IBA_ORB_MATCH_HISTO];
    int32_t ind[3];
} iba_orb_match_counts;
typedef struct iba_orb_matches iba_orb_matches;
iba_status iba_default_orb_match_options(iba_orb_match_options* opt);
const char* iba_orb_match_last_error(void);                          /* never NULL; of this thread's last iba_orb_match* call that failed */
/* *out is NULL on failure; release it with iba_orb_matches_free */
iba_status iba_orb_match(const iba_orb_frame* frames, int32_t F, const iba_orb_match_job* jobs, int32_t J, const iba_orb_match_options* opt, int device, iba_orb_matches** out);
void       iba_orb_matches_free(iba_orb_matches* m);
int32_t    iba_orb_matches_n_jobs(const iba_orb_matches* m);         /* 0 for NULL */
iba_status iba_orb_matches_job(const iba_orb_matches* m, int32_t job, iba_orb_match_counts* counts);
iba_status iba_orb_matches_read(const iba_orb_matches* m, int32_t job, int32_t* match /* n_queries */, int32_t* dist /* n_queries */);   /* either may be NULL */
/* stage accessors, keep_stages only. Grid: cell_off[3073] with cell = px * 48 + py (the order M3 walks) and list[cell_off[3072]] = the frame's keypoints
 * by cell, ascending inside a cell; *n_listed = cell_off[3072] (the keypoints that are in a cell). Lists: off[n_queries + 1] and, per entry, the train
 * index and the distance in M3's order; their length is the job's n_candidates. Every output may be NULL. */
iba_status iba_orb_matches_grid(const iba_orb_matches* m, int32_t frame, int32_t* cell_off /* 3073 */, int32_t* list /* cap n */, int32_t* n_listed);
iba_status iba_orb_matches_lists(const iba_orb_matches* m, int32_t job, int32_t* off /* n_queries + 1 */, int32_t* index, uint16_t* dist);
/* host only, pure functions: the per-query arrays of the reference's two call sites (rules above). The outputs take frame->n entries each. */
iba_status iba_orb_match_init_queries(const iba_orb_frame* frame1, const float* prev_matched_xy /* n x 2 */, int32_t window_size,
                                      float* centre_xy, float* radius, int32_t* level_range, int32_t* query_index, uint8_t* valid);
iba_status iba_orb_match_motion_queries(const iba_orb_frame* last_frame, const uint8_t* has_point /* n */, const uint8_t* outlier /* n */, const float* world_xyz /* n x 3 */,
                                        const float Tcw12[12] /* the current frame's */, float fx, float fy, float cx, float cy, const float bounds[4] /* the current frame's min_x max_x min_y max_y */,
                                        const float* scale_factors, int32_t n_scale_factors, float th,
                                        float* centre_xy, float* radius, int32_t* level_range, int32_t* query_index, uint8_t* valid);

/*
 * ---- Two-view initialisation [the camera side's third brick: the reference's Initializer::Initialize and everything it calls
 * (src/orb_slam/src/Initializer.cc: FindHomography :124, FindFundamental :175, ComputeH21 :226, ComputeF21 :268, CheckHomography :305, CheckFundamental
 * :390, ReconstructF :470, ReconstructH :572, Triangulate :734, Normalize :749, CheckRT :798, DecomposeE :909)] ----
 * A call takes B frame pairs on one device. A pair is the positions of both frames, the matches12 array (what iba_orb_matches_read returns in match for
 * an INIT job built by iba_orb_match_init_queries), the pinhole intrinsics and the RANSAC sets. The MATCH LIST is the pairs (i, matches12[i]) with
 * matches12[i] >= 0 in ascending i; N is its length. Per pair the call runs `iterations` hypotheses of a homography and of a fundamental matrix, scores
 * each over every match, picks a model by the score ratio, decomposes it into 8 or 4 motion hypotheses, triangulates every inlier under each and accepts
 * or refuses the pair. What Tracking::CreateInitialMapMonocular does after a success (global BA, median-depth scaling) and the >= 100-matches gates
 * around the call are the caller's.
 * ARITHMETIC. float32 wherever the reference's plain C++ is float, with the C++ promotions of the cited line: 1.0/(...) is a double division rounded to
 * float; 0.9*N, 0.7*maxGood, 0.75*bestGood and cosParallax<0.99998 compare in double; 4.0*mSigma2 is a double product rounded to float. Every operation
 * rounded, left to right, no contraction. Every cv::Mat operation (3 x 3 and 3 x 4 products, inv, determinant, norm, dot, the SVDs) is the library's
 * own restatement in float64 on the widened float32 entries, a fixed sequence of + - x / sqrt; each element that lands in a CV_32F matrix is rounded
 * once to float32. A product element is ((a0 b0 + a1 b1) + a2 b2); a product of three matrices is two products, left first, the intermediate rounded;
 * det = (a (e i - f h) - b (d i - f g)) + c (d h - e g); inv = the cofactors, each divided by det; norm = sqrt((x x + y y) + z z). A NaN stored
 * into Hi, H12i, Fi, a score or a cosine is stored as 0x7FC00000 (devices differ in the NaN they produce; no decision reads its bits).
 * tests/twoview_ref.py restates T1-T11 in numpy; the device results are compared byte for byte, parallax_deg within one float32 ulp.
 *
 *   T1 normalise.  (host, :749-795 exactly) over ALL keypoints of the frame, matched or not: the float32 sums meanX, meanY, meanDevX, meanDevY are
 *                  sequential in index order; mean = sum / n; sX = (float)(1.0 / meanDevX); out = (x - meanX) * sX; T = [sX 0 -meanX*sX; 0 sY
 *                  -meanY*sY; 0 0 1].
 *   T2 null vector. The right singular vector of the least singular value of an m x n matrix (16 x 9, 8 x 9, 4 x 4, 3 x 3) by one-sided (Hestenes)
 *                  Jacobi in float64: G = the float32 matrix widened, V = I; sweep the pairs p < q in row-cyclic order; alpha = sum g_p^2, beta =
 *                  sum g_q^2, gamma = sum g_p g_q over the rows in order; skip the pair iff gamma^2 <= alpha beta 2^-104, or alpha or beta <= 2^-104 x (the sum of
 *                  the squares of the matrix' entries, summed once in row-major order: a column at the rounding level of the matrix is null and rests;
 *                  without this clause every matrix of rank below n, the 8 x 9 ones, runs to the cap on its vanishing column); else zeta = (beta -
 *                  alpha) / (2 gamma), t = sign(zeta) / (|zeta| + sqrt(1 + zeta^2)) with sign(0) = +1, c = 1 / sqrt(1 + t^2), s = c t;
 *                  g_p' = c g_p - s g_q, g_q' = s g_p + c g_q, the same for V's columns. Stop after the first sweep that rotates nothing, after 30
 *                  sweeps at the latest (a debug counter reports that case). The answer is V's column under G's column of least squared norm, the
 *                  first on a tie, rounded to float32; its sign is whatever falls out (every consumer is sign-invariant or tries both signs). The
 *                  3 x 3 SVD of T4, T7, T8 is the same routine: w_k = sqrt of the squared column norms, sorted descending (stable), V's columns
 *                  with them, u_k = G's column / w_k; u_3 = u_1 x u_2 where w_3 <= 2^-23 w_1; u, w, vt rounded to float32.
 *   T3 H hypothesis. (:226-266, :159-161) A (16 x 9) from the 8 normalised pairs as written; Hn = T2's vector reshaped; H21i = T2inv Hn T1 with
 *                  T2inv = [1/sx 0 -tx/sx; 0 1/sy -ty/sy; 0 0 1] in closed form; H12i = inv of H21i. A singular H21i gives non-finite entries
 *                  which T5 scores as IEEE dictates.
 *   T4 F hypothesis. (:268-303, :212) Fpre from T2 on A (8 x 9); v3 = T2 on Fpre (3 x 3); Fn = Fpre - (Fpre v3) v3^T, which is what
 *                  u diag(w1, w2, 0) vt equals, without forming u; F21i = T2^T Fn T1.
 *   T5 scores.     CheckHomography :305-388 and CheckFundamental :390-468 in float32 exactly as written, th = 5.991f (3.841f and 5.991f),
 *                  invSigmaSquare = (float)(1.0 / (sigma * sigma)); the score is the SEQUENTIAL float32 sum over the matches in list order, the two
 *                  terms of a match interleaved. The order of that sum is part of the rule: it decides which iteration wins.
 *   T6 selection.  Per model the first iteration whose score is strictly greater than every earlier one, starting from 0.0f (a NaN score never
 *                  wins); none: best_it = -1 and the score 0. Its inlier flags are bIn of T5. RH = SH / (SH + SF) in float32 (0 where both are 0);
 *                  RH > rh_threshold takes the H path (model = 1). The chosen path's model having no iteration is status NO_MODEL.
 *   T7 motion from F. (:478-497, :909-929) E = K^T F K; the SVD of T2; t = u_3 / norm(u_3); R1 = U W Vt, R2 = U W^T Vt with W = [0 -1 0; 1 0 0;
 *                  0 0 1], each negated where its determinant is < 0. Hypotheses (R1, t), (R2, t), (R1, -t), (R2, -t) in that order.
 *   T8 motion from H. (:584-686 as written: Faugeras, 8 hypotheses, float32 scalars) A = inv(K) H21 K; the SVD of T2; s = (float)(det U * det Vt);
 *                  the early refusal (double)(d1/d2) < 1.00001 || (double)(d2/d3) < 1.00001 is status H_DEGENERATE; R = ((s U) Rp) Vt with s U
 *                  elementwise in float32; tp scaled in float32, t = U tp divided by its norm. The plane normals are not computed: nothing reads them.
 *   T9 CheckRT.    (:798-907, :734-747) per (motion hypothesis, inlier match of the chosen model): P1 = K [I | 0], P2 = K [R | t], O2 = -R^T t;
 *                  A's rows in float32 as written (x * P.row(2) - P.row(0), ...); x = T2 on A (4 x 4); p = x / x_3 in float32; then, in this order,
 *                  verdict 1: p not finite; dist1, dist2 (float32 of the float64 norms), cosParallax = (float)(dot / (double)(dist1 * dist2));
 *                  2: p_z <= 0 && cos < 0.99998; p2 = R p + t (one rounding per element); 3: p2_z <= 0 && cos < 0.99998; 4: squareError1 > th2;
 *                  5: squareError2 > th2 with th2 = (float)(4.0 * sigma^2); 6: good. 0 is a match that is no inlier of the chosen model. n_good
 *                  counts verdict 6. points is written for every good match, triangulated only where cos < 0.99998 as well: the reference's
 *                  behaviour. cos_parallax = the good cosines' value at sorted position min(50, n_good - 1) (ascending; 1.0f where n_good == 0,
 *                  which gives the reference's parallax 0); parallax_deg = (float)(acos((double)c) * 180 / pi), computed on the HOST.
 *   T10 acceptance. ReconstructF :499-569 and ReconstructH :689-731 as written: nMinGood = max((int)(0.9 * N), min_triangulated) with N = the chosen
 *                  model's inliers, nsimilar over n_good > 0.7 * maxGood, the else-if chain on equal counts (the FIRST hypothesis at maxGood),
 *                  parallax > min_parallax_deg in the first and >= in the second, secondBestGood < 0.75 * bestGood, bestGood > min_triangulated,
 *                  bestGood > 0.9 * N.
 *   T11 status.    OK; TOO_FEW_MATCHES (N < 8: the reference would draw from an empty list; the library's own rule, decided on the host);
 *                  NO_MODEL (T6); H_DEGENERATE (T8); NO_CLEAR_WINNER; TOO_FEW_POINTS; LOW_PARALLAX. Where the reference's single return false
 *                  covers several reasons the order of the tests in its code decides: F path maxGood < nMinGood (TOO_FEW_POINTS), nsimilar > 1
 *                  (NO_CLEAR_WINNER), the parallax (LOW_PARALLAX); H path the second-best test (NO_CLEAR_WINNER), the parallax (LOW_PARALLAX), the
 *                  two count tests (TOO_FEW_POINTS). chosen is the hypothesis whose parallax was tested (status OK, LOW_PARALLAX, or the H path's
 *                  TOO_FEW_POINTS), else -1. R21, t21, points and triangulated are zeros unless the status is OK; n_hyp is 0 where T7 / T8 were
 *                  not reached or refused.
 *
 * UNPINNED, together: every cv::Mat operation named under ARITHMETIC (OpenCV's gemm, inv, determinant, norm and its Jacobi SVD may round and order
 * otherwise; nothing here is compared with recorded OpenCV output), hence T2, and what T3, T4, T7, T8 and T9 build on it; the sign of every null
 * vector; the sets of iba_twoview_sets (the reference draws from DUtils::Random, C rand(), which is not vendored; sets is an INPUT so a caller can
 * hand in the reference's own); acos of the host's libm in parallax_deg; TOO_FEW_MATCHES. KNOWN DEVIATION: the reference compares RH with the double
 * 0.40, the library with the float32 option (0.40f): they differ for RH == 0.40f alone.
 * DEVICE (csrc/iba_twoview_kernels.hpp), one launch chain per chunk of pairs: hypotheses (one lane per (pair, iteration, model), T2's work matrices
 * in a lane-minor LDS slab); scores (one lane per hypothesis, a wave = 64 hypotheses of one pair and model, the match coordinates wave-uniform;
 * the sum stays in a register and is never reduced across lanes); selection (one wave per (pair, model), then the winner's inlier flags); motion
 * hypotheses (one lane per pair); CheckRT (one lane per (pair, hypothesis, match); n_good by ballot and integer atomics); the k-th cosine by a
 * radix select on the ordered keys (integer histograms in LDS); acceptance (one lane per pair); without keep_stages a gather of the candidate
 * hypothesis' per-match entries, so that only those come down. Only integer counts are combined by atomics. A
 * pair goes up once (32 bytes per match, 32 per set) and comes down once; T1, the set check and TOO_FEW_MATCHES are the host's before the device is touched.
 * MEMORY: a pair takes 187 bytes per match and 148 per iteration on the device while its chunk runs; a call is cut into chunks of consecutive pairs
 * (at most 32768) that stay under 1 GiB, or under a quarter of the device memory free at the call where that is less; a chunk holds at least one pair
 * and a chunk boundary changes no byte. The result is host memory.
 * ERRORS, all IBA_ERR_INVALID_ARG with a message (iba_twoview_last_error, per thread) BEFORE the device is touched: a NULL argument (a frame's arrays
 * may be NULL only where its n == 0; sets only where N < 8) or a wrong struct_size; B < 1; n1 or n2 < 0 or above IBA_ORB_MATCH_MAX_KEYPOINTS; a
 * match index >= n2; a position that is not finite; fx or fy not finite or <= 0, cx or cy not finite; sigma not finite or <= 0; iterations outside
 * 1..IBA_TWOVIEW_MAX_ITERATIONS; a set index outside [0, N) or repeated inside its set, for pairs with N >= 8; min_triangulated < 0; a threshold that
 * is not finite; a pair or hypothesis index outside the result; a stage accessor on a result without keep_stages. A pair with N < 8 is legal
 * (status), and so is n1 == 0.
 */
#define IBA_TWOVIEW_MAX_ITERATIONS 4096
typedef enum iba_twoview_status {
    IBA_TWOVIEW_OK = 0, IBA_TWOVIEW_TOO_FEW_MATCHES = 1, IBA_TWOVIEW_NO_MODEL = 2, IBA_TWOVIEW_H_DEGENERATE = 3, IBA_TWOVIEW_NO_CLEAR_WINNER = 4,
    IBA_TWOVIEW_TOO_FEW_POINTS = 5, IBA_TWOVIEW_LOW_PARALLAX = 6
} iba_twoview_status;
typedef struct iba_twoview_pair {             /* host pointers, read during the call only */
    const float*   xy1;        /* n1 x 2 */
    const float*   xy2;        /* n2 x 2 */
    const int32_t* matches12;  /* n1: an index into frame 2, or < 0 */
    const int32_t* sets;       /* iterations x 8 indices into the match list, distinct inside a set (iba_twoview_sets); NULL only where N < 8 */
    int32_t n1, n2;
    float fx, fy, cx, cy;
} iba_twoview_pair;
typedef struct iba_twoview_options {
    int32_t struct_size;        /* sizeof(iba_twoview_options) */
    float   sigma;              /* 1.0f */
    int32_t iterations;         /* 200, 1..IBA_TWOVIEW_MAX_ITERATIONS */
    float   min_parallax_deg;   /* 1.0f */
    int32_t min_triangulated;   /* 50 */
    float   rh_threshold;       /* 0.40f */
    int32_t keep_stages;        /* 0; 1 keeps every iteration's matrices and scores and every motion hypothesis' points and verdicts */
} iba_twoview_options;
typedef struct iba_twoview_result {
    int32_t status;             /* iba_twoview_status */
    int32_t n_matches;          /* N */
    int32_t model;              /* 0 = F, 1 = H */
    int32_t n_hyp;              /* 4, 8, or 0 */
    int32_t chosen;             /* -1: none */
    int32_t best_it_H, best_it_F;   /* -1: none */
    int32_t n_inliers_H, n_inliers_F;
    float SH, SF, RH;
    float H21[9], F21[9];
    int32_t n_good[8];
    float cos_parallax[8], parallax_deg[8];
    float R21[9], t21[3];
} iba_twoview_result;
typedef struct iba_twoview_batch iba_twoview_batch;
iba_status iba_default_twoview_options(iba_twoview_options* opt);
const char* iba_twoview_last_error(void);                            /* never NULL; of this thread's last iba_twoview* call that failed */
/* *out is NULL on failure; release it with iba_twoview_free */
iba_status iba_twoview_init(const iba_twoview_pair* pairs, int32_t B, const iba_twoview_options* opt, int device, iba_twoview_batch** out);
void       iba_twoview_free(iba_twoview_batch* r);
int32_t    iba_twoview_n_pairs(const iba_twoview_batch* r);          /* 0 for NULL */
iba_status iba_twoview_read(const iba_twoview_batch* r, int32_t pair, iba_twoview_result* result);
/* the match list (N x 2: index in frame 1, index in frame 2) and the chosen model's inlier flags (N bytes); either may be NULL */
iba_status iba_twoview_matches(const iba_twoview_batch* r, int32_t pair, int32_t* list, uint8_t* inlier);
/* of the chosen motion hypothesis, indexed by the keypoint of frame 1: points n1 x 3, triangulated n1 bytes; either may be NULL */
iba_status iba_twoview_points(const iba_twoview_batch* r, int32_t pair, float* points, uint8_t* triangulated);
/* stage accessors, keep_stages only; every output may be NULL. Per iteration Hi, H12i, Fi (iterations x 9 each) and the two scores (iterations each);
 * zeros for a pair with N < 8. Per motion hypothesis (0 <= hyp < 8; zeros at or above n_hyp) R, t, n_good, and per match of the list the triangulated
 * point (N x 3, zeros for verdicts 0 and 1) and the verdict code of T9 (N bytes). */
iba_status iba_twoview_iterations(const iba_twoview_batch* r, int32_t pair, float* Hi, float* H12i, float* Fi, float* score_H, float* score_F);
iba_status iba_twoview_hypothesis(const iba_twoview_batch* r, int32_t pair, int32_t hyp, float R[9], float t[3], int32_t* n_good, float* points, uint8_t* verdict);
/* host only, pure functions (precedents: iba_orb_plan, iba_orb_match_init_queries). T1 on n >= 0 positions: out_xy n x 2 and T (3 x 3 row-major);
 * n == 0 gives a T that is not finite, as the reference's would be. */
iba_status iba_twoview_normalize(const float* xy, int32_t n, float* out_xy, float T[9]);
/* the reference's draw-without-replacement loop (:82-97: swap with back, pop) over the library's OWN generator, splitmix64 on seed with
 * randi = next() % size (UNPINNED, see above): out takes iterations x 8 indices into a match list of N >= 8 entries */
iba_status iba_twoview_sets(int32_t N, int32_t iterations, uint64_t seed, int32_t* out);

/*
 * ---- Motion-only pose optimisation [the camera side's fourth brick: the reference's Optimizer::PoseOptimization (src/orb_slam/src/Optimizer.cc:409-616),
 * which its tracker calls after every windowed match: TrackWithMotionModel, TrackReferenceKeyFrame, TrackLocalMap, and up to three times per
 * candidate in Relocalization (Tracking.cc:774, 897, 939, 1470-1501)] ----
 * A call takes B independent jobs on one device. A job is a start pose Tcw (3 x 4 row-major, float64), n 3D-2D edges (world point, undistorted
 * keypoint position, the information of the keypoint's pyramid level) and the pinhole intrinsics. Per job the WHOLE schedule - `rounds` rounds of up
 * to `iterations` Levenberg-Marquardt iterations of up to 10 trials each, the inlier / outlier classification between the rounds - runs inside one
 * kernel: the host does nothing between the upload and the download. Only monocular edges (EdgeSE3ProjectXYZOnlyPose) are built: this pipeline has
 * mvuRight < 0 everywhere; STEREO EDGES ARE NOT PROVIDED.
 * ARITHMETIC. float64 on the widened float32 inputs; every operation rounded, left to right as written, no contraction, nothing but + - x / sqrt up
 * to a step of theta = pi (P6). A NaN stored into an output is stored as the canonical quiet NaN (0x7FF8000000000000, 0x7FC00000).
 * tests/pose_ref.py restates P1-P8 in numpy; device, host restatement (iba_debug_pose_host) and numpy agree byte for byte.
 *
 *   P1 edge.       p = R X + t: p_x = ((T00 X + T01 Y) + T02 Z) + T03, p_y and p_z likewise with rows 1 and 2. e_x = obs_x - ((fx p_x) / p_z + cx),
 *                  e_y = obs_y - ((fy p_y) / p_z + cy). chi2 = inv_sigma2 (e_x e_x + e_y e_y). The Jacobian is the analytic 2 x 6 of
 *                  EdgeSE3ProjectXYZOnlyPose::linearizeOplus, rotation columns first, with iz = 1 / p_z and iz2 = iz iz:
 *                    J00 = ((p_x p_y) iz2) fx   J01 = (-(1 + (p_x p_x) iz2)) fx   J02 = (p_y iz) fx      J03 = (-iz) fx   J04 = 0          J05 = (p_x iz2) fx
 *                    J10 = (1 + (p_y p_y) iz2) fy   J11 = (-((p_x p_y) iz2)) fy   J12 = (-(p_x iz)) fy   J13 = 0          J14 = (-iz) fy   J15 = (p_y iz2) fy
 *                  p_z <= 0 is NOT tested, because the reference does not test it: the non-finite chi2 that follows makes a trial fail (P5) as
 *                  IEEE dictates.
 *   P2 Huber.      As BaseUnaryEdge::constructQuadraticForm applies RobustKernelHuber: dsqr = delta delta; chi2 > dsqr: sq = sqrt(chi2), rho = (2 sq)
 *                  delta - dsqr, rho' = delta / sq; else (and in a round without the kernel) rho = chi2, rho' = 1. w = rho' inv_sigma2 scales the
 *                  information: H_pq += w (J0p J0q + J1p J1q) for p <= q, b_p -= w (J0p e_x + J1p e_y), with the zeros of J as literal factors; the
 *                  chi2 sum takes rho. The same way as iba_ba.
 *   P3 sums.       21 (H, upper triangle by rows) + 6 (b) + 1 (robust chi2) sums per linearisation; a trial takes the chi2 sum alone. The order is
 *                  a function of n alone: edge i belongs to lane i mod 256; a lane adds its ACTIVE edges in ascending index onto +0.0; the 256 lane
 *                  sums are combined by the balanced binary tree v[l] = v[2l] + v[2l + 1], eight levels. (Six levels are a wave's DPP sum, two the
 *                  four waves' partial sums through LDS.) It does not depend on the chunk, the grid, or whether the job's edges sat on chip.
 *   P4 solve.      A = H with lambda added on the diagonal; A dx = b by ldlt6_factor / ldlt6_apply (LDL^T without pivoting, the library's own; a pivot
 *                  that is not positive and finite fails). A failed factorisation is a failed trial with chi2 = DBL_MAX.
 *   P5 LM.         g2o's OptimizationAlgorithmLevenberg as iba_ba restates it. Iteration 0: lambda = 1e-5 x the largest |H_kk|, ni = 2. Per iteration
 *                  current = the chi2 sum at the pose, then trials: the step of P4, T' = P6, temp = the chi2 sum at T'; rho = (current - temp) /
 *                  scale with scale = 1e-3 + sum_k dx_k (lambda dx_k + b_k), k ascending (1e-3 alone after a failed factorisation); the factorisation
 *                  succeeded, rho > 0 and temp finite: accept T', t = 2 rho - 1, alpha = min(1 - (t t) t, 2/3), lambda *= max(1/3, alpha), ni = 2, current = temp; else lambda
 *                  *= ni, ni *= 2, and a lambda that is not finite ends the optimisation. Trials repeat while rho < 0, at most 10; the optimisation
 *                  ends after an iteration with 10 trials or rho == 0, or after `iterations` iterations.
 *   P6 update.     T' = Exp(dx) T with dx = (omega, upsilon), the pose kept as a 3 x 4 float64: s = (w0 w0 + w1 w1) + w2 w2; Re = (I + A O) + B O2,
 *                  V = (I + B O) + C O2 entry by entry with O = [omega]x and O2 = [-(w1 w1 + w2 w2), w0 w1, w0 w2; ., -(w0 w0 + w2 w2), w1 w2; ., .,
 *                  -(w0 w0 + w1 w1)]; te_r = (V_r0 u0 + V_r1 u1) + V_r2 u2; R' = Re R with ((a0 b0 + a1 b1) + a2 b2), t'_r = (((Re_r0 t0 + Re_r1
 *                  t1) + Re_r2 t2) + te_r). A = sin(th)/th, B = (1 - cos(th))/th^2, C = (th - sin(th))/th^3 are the library's own fixed series in s,
 *                  14 terms each (k = 0..13; the first omitted term at th = pi is below 2^-53 of the leading one), nested a = 1 - (s / d_k) a from k =
 *                  13 down to 3 with d_k = (2k + off - 1)(2k + off), off = 1, 2, 3, the last two steps (k = 2, 1) in double-double (Dekker's
 *                  two_sum / two_prod, + - x / only), then x 1, x 0.5, / 6. No transcendental on the device up to th = pi, no small-angle branch,
 *                  one bit pattern everywhere, each coefficient within one ulp of its leading term. s > the double nearest pi^2: libm's sin,
 *                  cos and sqrt; a debug counter (iba_debug_pose_big_steps) reports such steps and NO byte-for-byte claim covers them.
 *   P7 classification. After each round every edge, active or not, is evaluated at the round's final accepted pose: (float)chi2 > chi2_threshold
 *                  marks an outlier and deactivates the edge, otherwise it is active again (a NaN chi2 is no outlier, as in the reference). The
 *                  rule iba_ba uses.
 *   P8 schedule.   n < 3: nothing runs, n_inliers = 0, the pose is the start pose, rounds_run = 0. Every round restarts from the start pose with
 *                  the current active set (Optimizer.cc:542); rounds 0..robust_rounds-1 use the Huber kernel; n < 10 stops after the first round
 *                  (optimizer.edges().size() < 10). The result is the last round's pose, n_inliers = n - its n_bad. Per round: chi2 (the robust
 *                  sum over the round's active edges at its final pose), n_bad, lm_iterations (begun), trials.
 *   P9 edges from matches. (host only, pure) mCurrentFrame.mvpMapPoints[match[q]] = the last frame's point of query q, for the queries in ascending
 *                  order (a later query overwrites), then the loop of Optimizer.cc:445-484: the current frame's keypoints that hold a point in
 *                  ascending index give xyz, obs = the keypoint's position, inv_sigma2 = inv_level_sigma2[octave] and the keypoint's index
 *                  (vnIndexEdgeMono).
 *
 * UNPINNED, together (g2o is third party and absent): the Jacobian's association in P1, the Huber form of P2, all of P4 (g2o solves with Eigen's
 * Cholesky of the 6 x 6 block) and P5 (tau, rho, the clamp, ni, the stop), Exp of P6 (g2o's SE3Quat::exp branches at small theta and calls libm), and
 * the order of every sum. KNOWN DEVIATIONS: g2o keeps the pose as a normalised quaternion and Converter::toSE3Quat re-orthonormalises the float pose;
 * here the caller's Tcw12 is used as given and never re-orthonormalised. g2o's active edges can carry the errors of a rejected last trial into the
 * classification; P7 evaluates at the accepted pose.
 * DEVICE (csrc/iba_pose_kernels.hpp): one workgroup of 256 lanes per job, grid-stride over the jobs of a chunk, ONE launch per chunk. A job's edges
 * are loaded once into LDS (24 bytes and a flag each) up to IBA_POSE_ONCHIP_EDGES; the edges above that are re-read from global memory by the same
 * arithmetic. Per evaluation the lanes do their edges, the wave sums by DPP, the four partial sums meet in LDS, one lane solves and updates in LDS
 * and the new pose is broadcast through LDS. No atomics on floating-point values. iba_pose_eval is one linearisation by the same device functions.
 * Chunks of consecutive jobs run under 1 GiB, or a quarter of the free device memory where that is less; a chunk boundary changes no byte.
 * ERRORS, all IBA_ERR_INVALID_ARG with a message (iba_pose_last_error, per thread) BEFORE the device is touched: a NULL argument (a job's edge
 * arrays may be NULL only where n == 0) or a wrong struct_size; B < 1; n < 0 or above IBA_ORB_MATCH_MAX_KEYPOINTS; a pose, point, observation,
 * information or intrinsic that is not finite; fx or fy <= 0; inv_sigma2 < 0; rounds outside 1..8, iterations outside 1..100, robust_rounds outside
 * 0..8, a threshold or delta that is not finite, chi2_threshold < 0, huber_delta <= 0; a job or round index outside the result; the stage accessor
 * on a result without keep_stages. n == 0 is legal.
 */
#define IBA_POSE_ONCHIP_EDGES 1024
#define IBA_POSE_MAX_ROUNDS 8
typedef struct iba_pose_job {                 /* host pointers, read during the call only */
    const double* Tcw12;       /* 3 x 4 row-major: the start pose */
    const float*  xyz;         /* n x 3: MapPoint::GetWorldPos */
    const float*  obs;         /* n x 2: mvKeysUn[i].pt */
    const float*  inv_sigma2;  /* n: mvInvLevelSigma2[octave] */
    int32_t n;
    float fx, fy, cx, cy;
} iba_pose_job;
typedef struct iba_pose_options {
    int32_t struct_size;        /* sizeof(iba_pose_options) */
    int32_t rounds;             /* 4, 1..8 */
    int32_t iterations;         /* 10, 1..100 */
    float   chi2_threshold;     /* 5.991f */
    float   huber_delta;        /* (float)sqrt(5.991) */
    int32_t robust_rounds;      /* 3: the Huber kernel is off after this many rounds */
    int32_t keep_stages;        /* 0; 1 allows iba_pose_stage */
} iba_pose_options;
typedef struct iba_pose_result {
    int32_t n;
    int32_t n_inliers;          /* nInitialCorrespondences - nBad; 0 where n < 3 */
    int32_t rounds_run;
    int32_t reserved;
    double  Tcw12[12];
    float   Tcw12f[12];         /* the rounding of Converter::toCvMat */
    double  chi2[IBA_POSE_MAX_ROUNDS];
    int32_t n_bad[IBA_POSE_MAX_ROUNDS], lm_iterations[IBA_POSE_MAX_ROUNDS], trials[IBA_POSE_MAX_ROUNDS];
} iba_pose_result;
typedef struct iba_pose_batch iba_pose_batch;
iba_status iba_default_pose_options(iba_pose_options* opt);
const char* iba_pose_last_error(void);                               /* never NULL; of this thread's last iba_pose* call that failed */
/* *out is NULL on failure; release it with iba_pose_free */
iba_status iba_pose_optimize(const iba_pose_job* jobs, int32_t B, const iba_pose_options* opt, int device, iba_pose_batch** out);
/* one linearisation per job AT the job's Tcw12 (P1-P3, delta = (float)sqrt(5.991)): active is NULL (all edges of all jobs) or one pointer per job
 * (NULL = all, else n bytes); H is B x 36 (both triangles), b B x 6, chi2_robust B; chi2_edges is NULL or one pointer per job (NULL, or n doubles:
 * the chi2 of every edge, active or not) */
iba_status iba_pose_eval(const iba_pose_job* jobs, int32_t B, const uint8_t* const* active, int32_t robust, int device, double* H, double* b, double* chi2_robust,
                         double* const* chi2_edges);
void       iba_pose_free(iba_pose_batch* r);
int32_t    iba_pose_n_jobs(const iba_pose_batch* r);                 /* 0 for NULL */
iba_status iba_pose_read(const iba_pose_batch* r, int32_t job, iba_pose_result* result);
/* per edge the outlier flag and the float32 chi2 of the last classification (n each, zeros where n < 3); either may be NULL */
iba_status iba_pose_edges(const iba_pose_batch* r, int32_t job, uint8_t* outlier, float* chi2);
/* keep_stages only: the pose at the end of round `round` < rounds_run */
iba_status iba_pose_stage(const iba_pose_batch* r, int32_t job, int32_t round, double Tcw12[12]);
/* host only, pure (P9). match and query_index are those of the CLAIM job built by iba_orb_match_motion_queries (query_index NULL: query q is keypoint
 * q of the last frame); the outputs take up to n_cur entries each; *n is the number of edges */
iba_status iba_pose_edges_from_matches(const int32_t* match, const int32_t* query_index, int32_t n_queries, const float* last_world_xyz /* n_last x 3 */, int32_t n_last,
                                       const float* cur_xy /* n_cur x 2 */, const int32_t* cur_octave /* n_cur */, int32_t n_cur, const float* inv_level_sigma2, int32_t n_levels,
                                       float* xyz, float* obs, float* inv_sigma2, int32_t* keypoint_index, int32_t* n);

/*
 * ---- Local-map point matching [the camera side's sixth brick: the reference's Tracking::SearchLocalPoints (src/orb_slam/src/Tracking.cc:1141-1191):
 * Frame::isInFrustum (Frame.cc:269-325) for every local map point, then ORBmatcher::SearchByProjection(Frame&, const vector<MapPoint*>&, th)
 * (ORBmatcher.cc:45-137) on GetFeaturesInArea (rule M3), with MapPoint::PredictScale and the two distance bounds (MapPoint.cc:386-430)] ----
 * The step between iba_pose_optimize on the previous frame's matches and the second pose optimisation of TrackLocalMap: a frame is matched against
 * the MAP. A call takes F frames (iba_orb_frame, as iba_orb_match takes them), ONE table of P map points and J jobs; a job projects the points it
 * lists into one frame under one pose and matches those in view against the frame's keypoints. Frames and the point table go up once, however many
 * jobs name them. Float arithmetic is float32 unless a cast says otherwise, every operation rounded, evaluated left to right, no contraction;
 * tests/map_match_ref.py restates every rule in numpy, sequentially as the reference is written, and the device and the host restatement
 * (iba_debug_map_match_host) are compared with it byte for byte. The float decisions are ONE text, csrc/iba_map_match_math.hpp.
 *
 *   L1 frustum.    Per listed point, in list order. A point whose skip byte is set (the reference's isBad() and mnLastFrameSeen == the frame's id)
 *                  gets status SKIPPED and is not projected. Pc_i = ((R_i0 X + R_i1 Y) + R_i2 Z) + t_i with the job's Tcw12 (the order of
 *                  iba_orb_match_motion_queries). PcZ < 0.0f: DEPTH. invz = 1.0f / PcZ correctly rounded, formed as (float)(1.0 / (double)PcZ).
 *                  u = (fx * PcX) * invz + cx, v = (fy * PcY) * invz + cy. u or v not finite: NOT_FINITE (the library's own rule; the reference
 *                  lets a NaN through its comparisons; PcZ == +0 or -0 ends here). u < min_x || u > max_x || v < min_y || v > max_y of the frame's
 *                  bounds: BOUNDS (a centre exactly on a bound is kept). Ow_i = -((R_0i t_0 + R_1i t_1) + R_2i t_2), formed once per job; PO = P - Ow;
 *                  dist = (float)sqrt((PO_0^2 + PO_1^2) + PO_2^2) with the squares and sums in double (cv::norm). dist < 0.8f * min_dist || dist >
 *                  1.2f * max_dist: DISTANCE (exactly on a bound is kept). view_cos = (float)(((PO_0 n_0 + PO_1 n_1) + PO_2 n_2) / dist), all in
 *                  double (Mat::dot returns double). view_cos not finite or < view_cos_limit: ANGLE. ratio = max_dist / dist (float32, correctly
 *                  rounded). level = the least n with ratio <= scale_factors[n], n_levels - 1 where there is none; ratio <= 1 gives 0. Status
 *                  IN_VIEW carries u, v, view_cos and level.
 *   L2 query.      r = ((double)view_cos > 0.998) ? 2.5f : 4.0f (the comparison is in double because the reference's literal is a double: view_cos
 *                  == (float)0.998 lies above it); if (th != 1.0f) r *= th; radius = r * scale_factors[level]; levels (level - 1, level).
 *   L3 list.       The candidate list is M3's on the frame's grid (M2) with that centre, radius and levels; the distances are M4 against the
 *                  point's descriptor.
 *   L4 resolve.    Per keypoint of the frame a claimed bit, set at the start where the job's occupied byte is (the reference's mvpMapPoints[idx]
 *                  && Observations() > 0). The in-view points in list order: over the candidates that are not claimed and whose distance is below
 *                  256, take the two lexicographic minima of (distance, list position): (best, level1, idx) and (best2, level2), the levels being
 *                  the candidates' octaves. A missing slot is (256, -1). Accept iff a first was found, best <= th_high and not (level1 == level2 &&
 *                  (float)best > nn_ratio * (float)best2). On accept: claim the keypoint, match[point] = keypoint, dist[point] = best,
 *                  point_of[keypoint] = the point's list position. This overload has no rotation check.
 *                  WHY THE TWO MINIMA ARE THE REFERENCE'S SCAN. The reference keeps (bestDist, bestLevel, bestIdx) and (bestDist2, bestLevel2),
 *                  starts both at (256, -1) and walks the list with `if (dist < bestDist) {second = first; first = this} else if (dist <
 *                  bestDist2) {second = this}`. Invariant: after any prefix, first and second are the two least (distance, position) pairs of the
 *                  prefix below 256. A new candidate has the largest position so far. dist < bestDist: it is the new least pair and the old first,
 *                  which was below the old second, is the new second. Else dist >= bestDist, so it follows the first; dist < bestDist2 puts it
 *                  before the old second, so it is the new second. Else dist >= bestDist2 and a larger position: it follows both, nothing changes.
 *                  A candidate at 256 passes neither strict test. (Where no candidate is left the reference would index mvpMapPoints[-1] if it
 *                  accepted; `a first was found` is the library's guard and changes nothing for th_high < 256.)
 *   L5 outputs per job. Per listed point: status (uint8), u, v, view_cos, level, radius (zeros where not in view), match (the keypoint or -1), dist
 *                  (the accepted distance or -1). Per keypoint of the frame: point_of (the position in the job's list that claimed it, or -1).
 *                  Counts: one per status (status[IN_VIEW] is the reference's nToMatch), n_candidates (the sum of the list lengths), n_matches.
 *                  With keep_stages the candidate lists as iba_orb_matches_lists gives them.
 *   L6 edges.      (iba_map_match_pose_edges, host only, pure) the joining helper to iba_pose_job: the frame's keypoints in ascending index; a
 *                  keypoint that was claimed in the call (point_of >= 0) holds points[point_of]; else one that had a point before the call
 *                  (prior_point, table indices or -1) holds that; every such keypoint yields one edge: xyz from the table, obs = the keypoint's
 *                  position, inv_sigma2 = inv_level_sigma2[octave] and the keypoint's index, as iba_pose_edges_from_matches does for a CLAIM job.
 *
 * UNPINNED, together: the order of the sums of Pc and Ow (the reference forms them with OpenCV's 3 x 3 float product), dist (cv::norm's own
 * accumulation) and the dot product. KNOWN DEVIATIONS: (1) the level: the reference takes ceil(log(ratio) / mfLogScaleFactor) through libm, clamped to
 * [0, n_levels - 1]; the table rule gives the same integer except where ratio lies within rounding of a table entry, and keeps transcendentals off
 * the device, as P6 does (profiles/map_match_parity.md counts the differences on the test scene). (2) As in M7 every claim of the call counts,
 * where the reference skips a claimed keypoint only if its map point has Observations() > 0. (3) NOT_FINITE, above.
 * NOT PROVIDED: stereo (mvuRight, mTrackProjXR), the KeyFrame and Sim3 overloads of SearchByProjection, the BoW matchers, UpdateLocalMap
 * (choosing the local points and their order is the caller's) and the IncreaseVisible / IncreaseFound bookkeeping (the statuses and matches say
 * which points it applies to).
 * DEVICE (csrc/iba_map_match_kernels.hpp). Before the chunks, over the whole call: the frustum kernel - a flat table of (job, list position)
 * slots, one lane per slot, blocks that do not straddle a job so that pose, intrinsics, bounds and scale table are uniform per block; it writes the
 * status and the slot's query record, and counts the statuses by wave ballot into LDS with one integer atomic per counter and block; then the
 * matcher's own grid kernels (cell, scan, ordered fill) and its list kernel counting every slot's list - the point descriptors lie behind the
 * keypoint descriptors in the one flat descriptor table, so that kernel is unchanged. Per chunk of consecutive jobs: scan, the list kernel writing
 * candidates and distances, and the resolve kernel: ONE wave per job, because L4 is sequential; the claimed state is a bitmap in LDS (32768 keypoints
 * take 4 KB: there is no global fallback) seeded from occupied; the lanes stride over a point's segment keeping their two least keys, the wave's
 * first is a 64-bit key minimum and its second the least of the winner lane's second and the other lanes' firsts; lane 0 reads the two octaves and
 * applies the acceptance; one barrier follows each point with a non-empty segment. No floating-point atomics, no order depends on atomic arrival.
 * MEMORY: the candidate lists (IBA_MAP_MATCH_BYTES_PER_CANDIDATE bytes per entry, sized from the count pass) are cut into chunks of consecutive
 * jobs under IBA_MAP_MATCH_BUDGET_BYTES, or under a quarter of the device memory free at the call where that is less; a chunk holds at least one job
 * and a chunk boundary changes no byte. A chunk whose lists hold 2^31 entries or more answers IBA_ERR_UNSUPPORTED. The result is host memory.
 * ERRORS, all IBA_ERR_INVALID_ARG with a message (iba_map_match_last_error, per thread) BEFORE the device is touched: a NULL argument (the table's
 * arrays may be NULL only where P == 0; skip and occupied may always be NULL; points may be NULL only where n_points == P: all P in order) or a
 * wrong struct_size; J < 1, F < 1, P < 0; a frame that iba_orb_match would refuse; a job's frame or a listed point out of range; n_points < 0; a
 * pose entry, point, normal, distance, intrinsic or th that is not finite or whose magnitude is above 1e6; n_levels outside [1,
 * IBA_MAP_MATCH_MAX_LEVELS]; a scale table that is not finite, does not start at 1 or does not ascend strictly; th_high outside [0, 256]; nn_ratio
 * not finite or <= 0; view_cos_limit not finite; a job index outside the result; the stage accessor on a result without keep_stages. A job with
 * n_points == 0 and a frame with n == 0 are legal.
 */
#define IBA_MAP_MATCH_BUDGET_BYTES (1ull << 30)
#define IBA_MAP_MATCH_BYTES_PER_CANDIDATE 6ull
#define IBA_MAP_MATCH_MAX_LEVELS 64
#define IBA_MAP_MATCH_N_STATUS 7
typedef enum iba_map_match_status {
    IBA_MAP_MATCH_IN_VIEW = 0, IBA_MAP_MATCH_SKIPPED = 1, IBA_MAP_MATCH_DEPTH = 2, IBA_MAP_MATCH_NOT_FINITE = 3, IBA_MAP_MATCH_BOUNDS = 4, IBA_MAP_MATCH_DISTANCE = 5,
    IBA_MAP_MATCH_ANGLE = 6
} iba_map_match_status;
typedef struct iba_map_points {               /* host pointers, read during the call only */
    const float*   xyz;        /* n x 3: MapPoint::GetWorldPos */
    const float*   normal;     /* n x 3: MapPoint::GetNormal */
    const float*   min_dist;   /* n: mfMinDistance, raw (L1 applies the 0.8f) */
    const float*   max_dist;   /* n: mfMaxDistance, raw (L1 applies the 1.2f) */
    const uint8_t* desc;       /* n x 32: MapPoint::GetDescriptor */
    int32_t n;
} iba_map_points;
typedef struct iba_map_match_job {            /* host pointers, read during the call only */
    int32_t frame;                  /* index into the call's frame array */
    int32_t n_levels;               /* entries of scale_factors, 1..IBA_MAP_MATCH_MAX_LEVELS */
    int32_t n_points;
    float   th;
    float   fx, fy, cx, cy;
    const float*   Tcw12;           /* 3 x 4 row-major float32: the frame's mTcw */
    const float*   scale_factors;   /* n_levels: the frame's mvScaleFactors, [0] == 1, ascending */
    const int32_t* points;          /* n_points indices into the table in the order of mvpLocalMapPoints, or NULL: all P in order */
    const uint8_t* skip;            /* n_points, or NULL: none */
    const uint8_t* occupied;        /* one byte per keypoint of the frame, or NULL: none */
} iba_map_match_job;
typedef struct iba_map_match_options {
    int32_t struct_size;        /* sizeof(iba_map_match_options) */
    int32_t th_high;            /* 100 */
    float   nn_ratio;           /* 0.8f: the ORBmatcher of SearchLocalPoints */
    float   view_cos_limit;     /* 0.5f */
    int32_t keep_stages;        /* 0; 1 keeps the candidate lists for iba_map_matches_lists */
} iba_map_match_options;
typedef struct iba_map_match_counts {
    int32_t n_points;
    int32_t status[IBA_MAP_MATCH_N_STATUS];   /* by iba_map_match_status; status[IBA_MAP_MATCH_IN_VIEW] = nToMatch */
    int32_t n_candidates, n_matches;
} iba_map_match_counts;
typedef struct iba_map_matches iba_map_matches;
iba_status iba_default_map_match_options(iba_map_match_options* opt);
const char* iba_map_match_last_error(void);                          /* never NULL; of this thread's last iba_map_match* call that failed */
/* *out is NULL on failure; release it with iba_map_matches_free */
iba_status iba_map_match(const iba_orb_frame* frames, int32_t F, const iba_map_points* points, const iba_map_match_job* jobs, int32_t J, const iba_map_match_options* opt, int device,
                         iba_map_matches** out);
void       iba_map_matches_free(iba_map_matches* m);
int32_t    iba_map_matches_n_jobs(const iba_map_matches* m);         /* 0 for NULL */
iba_status iba_map_matches_job(const iba_map_matches* m, int32_t job, iba_map_match_counts* counts);
/* L5 per listed point, n_points entries each; any may be NULL */
iba_status iba_map_matches_read(const iba_map_matches* m, int32_t job, uint8_t* status, float* u, float* v, float* view_cos, int32_t* level, float* radius, int32_t* match, int32_t* dist);
/* L5 per keypoint of the job's frame (frame n entries) */
iba_status iba_map_matches_keypoints(const iba_map_matches* m, int32_t job, int32_t* point_of);
/* keep_stages only: off[n_points + 1] and, per entry, the keypoint and the distance in M3's order; their length is the job's n_candidates. Every
 * output may be NULL. */
iba_status iba_map_matches_lists(const iba_map_matches* m, int32_t job, int32_t* off, int32_t* index, uint16_t* dist);
/* host only, pure (L6). prior_point and point_of may be NULL (none); points NULL: list position k is table point k, and n_points must be P; the
 * outputs take up to n_kp entries each; *n is the number of edges */
iba_status iba_map_match_pose_edges(const int32_t* prior_point /* n_kp */, const int32_t* point_of /* n_kp */, const int32_t* points /* n_points */, int32_t n_points,
                                    const float* table_xyz /* P x 3 */, int32_t P, const float* xy /* n_kp x 2 */, const int32_t* octave /* n_kp */, int32_t n_kp,
                                    const float* inv_level_sigma2, int32_t n_levels, float* xyz, float* obs, float* inv_sigma2, int32_t* keypoint_index, int32_t* n);

/*
 * ---- New-map-point creation [the camera side's seventh brick: the reference's LocalMapping::CreateNewMapPoints (src/orb_slam/src/LocalMapping.cc:
 * 206-451) with ORBmatcher::SearchForTriangulation (ORBmatcher.cc:657-823), CheckDistEpipolarLine (:140-157) and ComputeF12 (LocalMapping.cc:535-552)] ----
 * The step that makes the map grow: for a new keyframe and its best covisible neighbours, match the keypoints that have no map point under the
 * epipolar constraint, triangulate every match and keep the points that pass the parallax, depth, reprojection and scale gates. A call takes F frames
 * (iba_orb_frame, as iba_orb_match takes them; xy is mvKeysUn), K keyframes (a frame under a pose, with the DBoW2::FeatureVector node of every
 * keypoint, the has-point bytes and the scene median depth) and J jobs (a current keyframe and its neighbours in the order of
 * GetBestCovisibilityKeyFrames). Frames and keyframes go up once, however many jobs name them.
 * THREE FACTS OF THE REFERENCE make every (job, neighbour, keypoint) outcome independent. (1) CreateNewMapPoints builds its matcher as
 * ORBmatcher matcher(0.6,false): there is no rotation histogram. (2) This reference's SearchForTriangulation never sets vbMatched2: several
 * keypoints of keyframe 1 may take the same keypoint of keyframe 2, and a query's result does not depend on any other query. (3) The only coupling
 * between neighbours is that a keypoint of the current keyframe that got a point from neighbour i is skipped for the neighbours > i; both
 * pKF2->AddMapPoint and mpCurrentKeyFrame->AddMapPoint happen after that neighbour's whole search. Hence the reference's sequential result is "the
 * first neighbour in order whose outcome is a success", and later successes of the same keypoint are what the reference would never have searched (R7).
 * JOBS ARE INDEPENDENT: each starts from the has_point bytes as given, even where two jobs name the same keyframe. Whoever wants the reference's
 * keyframe-after-keyframe sequence makes one call per step and sets the bytes of the created points in between.
 * Float arithmetic is float32 unless a cast says otherwise, every operation rounded, evaluated left to right, no contraction; tests/triangulate_ref.py
 * restates every rule in numpy, sequentially as the reference is written (neighbour after neighbour, with a has_point array it updates after each),
 * and the device and the host restatement (iba_debug_triangulate_host) are compared with it byte for byte. The float decisions are ONE text,
 * csrc/iba_triangulate_math.hpp. The thresholds are options held as float32; where the reference's literal is a double the option is WIDENED to
 * double and the comparison made in double (stated per rule; the widened float differs from the double literal by at most 2^-25 relative, so e.g.
 * a ratio of exactly 0.01f is kept where the reference, comparing against the double 0.01 just above it, skips).
 *
 *   R1 pair prologue. Per (job, neighbour). Ow of both keyframes as L1 forms it. baseline = (float)sqrt((b_0^2 + b_1^2) + b_2^2) in double over the
 *                  float32 differences b = Ow2 - Ow1. The neighbour is skipped, and every slot of it has status PAIR_SKIPPED, where
 *                  (double)(baseline / median_depth) < (double)min_baseline_ratio (the reference's literal 0.01 is a double; the quotient is
 *                  float32, correctly rounded). F12 = K1^-T [t12]x R12 K2^-1 with R12 = R1w R2w^T, t12 = -(R12 t2w) + t1w, the 3 x 3 products,
 *                  inverses and transposes those of csrc/iba_twoview_math.hpp (mul33, mul331, inv33, transpose33: float64 on the widened entries, one
 *                  rounding per element), associated ((K1^T)^-1 [t12]x) R12) K2^-1. The epipole in image 2, literally: C2 = R2w Ow1 + t2w, invz =
 *                  1.0f / C2z, ex = fx2 * C2x * invz + cx2, ey = fy2 * C2y * invz + cy2; an epipole that is not finite makes R3's comparison
 *                  false and gates nothing.
 *   R2 queries.    The queries are the keypoints of the current keyframe without a point and with node >= 0. The candidates of a query are the
 *                  keypoints of the neighbour with the same node, in ascending index; one that has a point is walked past. A keypoint that has a
 *                  point has status HAS_POINT. A query whose node does not occur among the neighbour's keypoints (with or without a point), and a
 *                  keypoint with node < 0, has status NO_NODE. (The reference walks the nodes ascending and inside a node the keypoints ascending,
 *                  so the flat node array fixes the whole feature vector; by fact (2) the order of the queries changes nothing.)
 *   R3 pick.       Walk the candidates in order with bestDist = th_low. A candidate is EXAMINED iff dist <= th_low && dist <= bestDist (dist = the
 *                  256-bit Hamming distance, M4). It is TAKEN iff it passes two checks. It is not inside the epipole gate: dx = ex - x2, dy = ey -
 *                  y2, refused where dx * dx + dy * dy < epipole_gate * scale_factors[octave2], in float32. And the epipolar line test: a = x1 *
 *                  F12_00 + y1 * F12_10 + F12_20, b and c likewise with the second and third column, num = a * x2 + b * y2 + c, den = a * a + b * b,
 *                  all float32 as written; den == 0 fails; dsqr = num * num / den; passes iff (double)dsqr < (double)chi2_line *
 *                  (double)level_sigma2[octave2] (the reference's 3.84 is a double). A taken candidate sets bestDist = dist. Because dist > bestDist
 *                  is what refuses a candidate, AN EQUAL DISTANCE REPLACES. No candidate taken: NO_MATCH.
 *                  WHY THE WALK IS A MINIMUM. Call a candidate ELIGIBLE iff dist <= th_low and it passes both checks; the checks do not depend on
 *                  bestDist. Invariant: after any prefix, bestDist is the least distance of the prefix's eligible candidates (th_low where there is
 *                  none) and the held candidate is the LAST eligible one of the prefix at that distance. A new candidate that is not eligible is
 *                  either not examined or examined and not taken; nothing changes. An eligible one with dist > bestDist is not examined; it is not
 *                  a minimum, nothing changes. An eligible one with dist <= bestDist is examined and taken: it is at the new least distance and it
 *                  is the last so far. So the walk yields the lexicographic minimum of (distance, DESCENDING position) over the eligible
 *                  candidates, which the device reduces in parallel as the minimum of the key (dist << 32) | (0xFFFFFFFF - position).
 *   R4 rays.       xn = ((x - cx) * invfx, (y - cy) * invfy, 1) with invfx = 1.0f / fx correctly rounded; ray = Rwc xn (mul331 with the transposed
 *                  rotation). cos = (float)(dot / (norm1 * norm2)), all in double. The match is triangulated iff cos > 0 && (double)cos <
 *                  (double)max_cos_parallax (the reference's 0.9998 is a double); otherwise PARALLAX.
 *   R5 triangulation. The rows of the 4 x 4 matrix A are xn1_0 Tcw1[2] - Tcw1[0], xn1_1 Tcw1[2] - Tcw1[1] and the same two of keyframe 2, in float32,
 *                  widened to double. The null vector is tv::null_vector<4,4,1,1>, the Jacobi of T9. x[3] == 0, or a quotient that is not finite:
 *                  DEGENERATE (the library's guard; the reference tests only x[3] == 0). x3D = x[0..2] / x[3], correctly rounded.
 *   R6 gates, in the reference's order. z_i = (float)(((R_20 X + R_21 Y) + R_22 Z) + t_2) in double (Mat::dot returns double), x_i and y_i likewise.
 *                  (1) z1 <= 0: DEPTH1. (2) z2 <= 0: DEPTH2. (3) invz = (float)(1.0 / (double)z1), u = fx * x * invz + cx, v = fy * y * invz + cy, err2 =
 *                  (u - kp_x)^2 + (v - kp_y)^2 in float32; (double)err2 > (double)chi2_mono * (double)level_sigma2[octave1]: REPROJ1 (5.991 is a
 *                  double). (4) the same in keyframe 2: REPROJ2. (5) dist_i = (float)|x3D - Ow_i| (float32 differences, the norm in double); dist1 ==
 *                  0 || dist2 == 0: ZERO_DIST. (6) ratioDist = dist2 / dist1, ratioOctave = scale_factors[octave1] / scale_factors[octave2], both
 *                  correctly rounded, ratioFactor = 1.5f * scale_factor; ratioDist * ratioFactor < ratioOctave || ratioDist > ratioOctave *
 *                  ratioFactor: SCALE. (7) Otherwise CREATED.
 *   R7 first neighbour wins. Per keypoint of the current keyframe, the neighbours in order: every slot AFTER the keypoint's first CREATED neighbour
 *                  is SUPERSEDED, with match -1, dist -1 and xyz zero, whatever its own outcome (a later success, a NO_MATCH, a PAIR_SKIPPED): it is
 *                  the has-point the reference would have seen. Slots up to and including the first CREATED one keep their outcome.
 *   R8 the new point. xyz is the triangulated point; desc the current keyframe's descriptor of idx1; normal = (n1 + n2) * 0.5f with n_i,k =
 *                  (float)((double)(x - Ow_i)_k / |x - Ow_i|), the current keyframe first; max_dist = (float)|x - Ow_1| * scale_factors[octave1];
 *                  min_dist = max_dist / scale_factors[n_levels - 1], correctly rounded. The created points of a job come in the reference's
 *                  creation order: neighbour order first, ascending idx1 inside a neighbour.
 *
 * OUTPUTS per job: per (neighbour, keypoint of the current keyframe) slot, neighbour-major: status (uint8), match (idx2 or -1), dist (or -1), xyz
 * (zeros unless R5 produced a point; kept for the refusals of R6). Counts: one per status, and per neighbour n_matches (the reference's nmatches of
 * that round: the taken slots that are not SUPERSEDED) and n_created. The created points with idx1, the neighbour's position, idx2 and the five
 * arrays of an iba_map_points table: a caller appends them to its table as they are. With keep_stages the length of every slot's candidate segment.
 * UNPINNED: the sums of F12, the epipole, the rays and the projections (the reference forms them with OpenCV's float products), cv::norm's
 * accumulation, cv::SVD against the Jacobi. KNOWN DEVIATIONS: (1) the widened float thresholds, above. (2) The reference's
 * ComputeDistinctiveDescriptors and the order of the normal sum in UpdateNormalAndDepth follow the pointer order of a std::map<KeyFrame*, size_t>;
 * R8 fixes both (with two observations at distance d the median rule picks either descriptor: profiles/triangulate_parity.md counts the points
 * for which the other order would differ). (3) DEGENERATE for a quotient that is not finite. Once a created point has a third observation, its
 * descriptor, normal and bounds come from iba_refresh (S1-S7 below), which gives R8's bytes for the two observations listed current keyframe first.
 * GUARDS. Under the default options DEGENERATE and ZERO_DIST are guards, as their tests are in the reference: x[3] == 0 needs parallel rays, which
 * are PARALLAX first, and x3D == Ow_i makes z_i = r_2 . (x3D - Ow_i) zero, which is DEPTH1 / DEPTH2 first. REPROJ2 needs a candidate further than
 * sqrt(chi2_mono) sigma from the reprojection yet nearer than sqrt(chi2_line) sigma, of the same octave, to the line, and the triangulated point
 * reprojects between the two. tests/triangulate_scene.py reaches DEGENERATE and REPROJ2 with max_cos_parallax and chi2_line opened, the self-test
 * ZERO_DIST with a hand-made centre.
 * NOT PROVIDED: stereo (mvuRight, bOnlyStereo, UnprojectStereo), mbCheckOrientation = true, the CheckNewKeyFrames() early return, the choice of
 * neighbours, computing the node ids (DBoW2). iba_triangulate_median_depth (host only, pure) is
 * KeyFrame::ComputeSceneMedianDepth: z = (float)dot + zcw with the dot of the pose's third row and the point in double, sorted ascending, element
 * (n - 1) / q.
 * DEVICE (csrc/iba_triangulate_kernels.hpp). The node order of every keyframe - its keypoints with node >= 0 sorted by (node, index) - is a host
 * sort uploaded with the keyframes: the node array is read on the host for the checks anyway, a keyframe has a few thousand keys, and the sorted
 * table is then an input like the frames, with no temporary storage and no further library on the device. Per chunk of consecutive jobs over flat
 * tables: the prologue kernel (one lane per pair, R1); the segment kernel (one lane per slot, blocks that do not straddle a pair; binary search of the
 * neighbour's sorted keys; writes HAS_POINT, NO_NODE, PAIR_SKIPPED where a slot ends); the pick kernel (W lanes per query, W = 8, 16 or 64: the
 * query's 256 bits in registers, the lanes stride over the segment and keep their least key, the group minimum by xor shuffles inside the group);
 * compaction of the matched slots by ballot prefix with one integer atomic per block for the base, and the triangulate kernel, one lane per
 * matched slot, writing by slot index so that arrival order changes no byte; the resolve kernel, one lane per (job, keypoint), R7; counts by ballot
 * with integer atomics, a scan over the blocks and the gather of the created points in R8's order. No floating-point atomics, and no result
 * depends on the arrival order of an atomic.
 * MEMORY: IBA_TRIANGULATE_BYTES_PER_SLOT bytes per slot; a call is cut into chunks of consecutive jobs under IBA_TRIANGULATE_BUDGET_BYTES, or under
 * a quarter of the device memory free at the call where that is less; a chunk holds at least one job and a chunk boundary changes no byte. 2^31
 * slots or more in a call answer IBA_ERR_UNSUPPORTED. The result is host memory.
 * ERRORS, all IBA_ERR_INVALID_ARG with a message (iba_triangulate_last_error, per thread) BEFORE the device is touched: a NULL argument (has_point
 * may always be NULL, node only where the frame has n == 0, neighbours only where n_neighbours == 0) or a wrong struct_size; J < 1, K < 1, F < 1; a
 * frame that iba_orb_match would refuse; a keyframe's frame, a job's current or a neighbour out of range; a neighbour equal to current or listed
 * twice; n_neighbours < 0; a pose entry or intrinsic that is not finite or whose magnitude is above 1e6; a median_depth that is not finite or <= 0
 * on a keyframe used as a neighbour; n_levels outside [1, IBA_TRIANGULATE_MAX_LEVELS]; a scale table that is not finite, does not start at 1 or does
 * not ascend strictly; a level_sigma2 or scale_factor that is not finite, above 1e6 or <= 0; an octave of a keyframe of the job outside [0, n_levels);
 * th_low outside [0, 256]; a float threshold that is not finite; a job index outside the result; the stage accessor on a result without
 * keep_stages; iba_triangulate_median_depth with n < 1 (the reference would index out of bounds) or q < 1. n_neighbours == 0 and frames with n == 0
 * are legal.
 */
#define IBA_TRIANGULATE_BUDGET_BYTES (1ull << 30)
#define IBA_TRIANGULATE_BYTES_PER_SLOT 120ull
#define IBA_TRIANGULATE_MAX_LEVELS 64
#define IBA_TRIANGULATE_N_STATUS 14
typedef enum iba_triangulate_status {
    IBA_TRIANGULATE_CREATED = 0, IBA_TRIANGULATE_HAS_POINT = 1, IBA_TRIANGULATE_NO_NODE = 2, IBA_TRIANGULATE_PAIR_SKIPPED = 3, IBA_TRIANGULATE_NO_MATCH = 4,
    IBA_TRIANGULATE_PARALLAX = 5, IBA_TRIANGULATE_DEGENERATE = 6, IBA_TRIANGULATE_DEPTH1 = 7, IBA_TRIANGULATE_DEPTH2 = 8, IBA_TRIANGULATE_REPROJ1 = 9,
    IBA_TRIANGULATE_REPROJ2 = 10, IBA_TRIANGULATE_ZERO_DIST = 11, IBA_TRIANGULATE_SCALE = 12, IBA_TRIANGULATE_SUPERSEDED = 13
} iba_triangulate_status;
typedef struct iba_triangulate_keyframe {     /* host pointers, read during the call only */
    int32_t frame;                  /* index into the call's frame array */
    float   fx, fy, cx, cy;
    float   median_depth;           /* ComputeSceneMedianDepth(2) of this keyframe; used only where it is a neighbour */
    const float*   Tcw12;           /* 3 x 4 row-major float32 */
    const int32_t* node;            /* n of the frame: the DBoW2::FeatureVector node of every keypoint, < 0: in no node */
    const uint8_t* has_point;       /* n bytes, or NULL: none has a point */
} iba_triangulate_keyframe;
typedef struct iba_triangulate_job {          /* host pointers, read during the call only */
    int32_t current;                /* index into the call's keyframe array */
    int32_t n_neighbours;
    int32_t n_levels;               /* entries of scale_factors and level_sigma2, 1..IBA_TRIANGULATE_MAX_LEVELS */
    float   scale_factor;           /* mfScaleFactor */
    const int32_t* neighbours;      /* n_neighbours indices into the keyframe array, distinct, none equal to current */
    const float*   scale_factors;   /* n_levels: mvScaleFactors, [0] == 1, ascending */
    const float*   level_sigma2;    /* n_levels: mvLevelSigma2 */
} iba_triangulate_job;
typedef struct iba_triangulate_options {
    int32_t struct_size;        /* sizeof(iba_triangulate_options) */
    int32_t th_low;             /* 50 */
    float   min_baseline_ratio; /* 0.01f, widened (R1) */
    float   max_cos_parallax;   /* 0.9998f, widened (R4) */
    float   epipole_gate;       /* 100.f (R3, float32) */
    float   chi2_line;          /* 3.84f, widened (R3) */
    float   chi2_mono;          /* 5.991f, widened (R6) */
    int32_t keep_stages;        /* 0; 1 keeps the segment lengths for iba_triangulation_segments */
} iba_triangulate_options;
typedef struct iba_triangulate_counts {
    int32_t n_keypoints;        /* of the current keyframe */
    int32_t n_neighbours;       /* the job's slots are n_neighbours x n_keypoints, neighbour-major */
    int32_t status[IBA_TRIANGULATE_N_STATUS];   /* by iba_triangulate_status, over the job's slots */
    int32_t n_created;          /* = status[IBA_TRIANGULATE_CREATED]: the points of iba_triangulation_points */
} iba_triangulate_counts;
typedef struct iba_triangulation iba_triangulation;
iba_status iba_default_triangulate_options(iba_triangulate_options* opt);
const char* iba_triangulate_last_error(void);                        /* never NULL; of this thread's last iba_triangulat* call that failed */
/* *out is NULL on failure; release it with iba_triangulation_free */
iba_status iba_triangulate(const iba_orb_frame* frames, int32_t F, const iba_triangulate_keyframe* keyframes, int32_t K, const iba_triangulate_job* jobs, int32_t J,
                           const iba_triangulate_options* opt, int device, iba_triangulation** out);
void       iba_triangulation_free(iba_triangulation* t);
int32_t    iba_triangulation_n_jobs(const iba_triangulation* t);     /* 0 for NULL */
/* the counts; n_matches and n_created take n_neighbours entries each and may be NULL */
iba_status iba_triangulation_job(const iba_triangulation* t, int32_t job, iba_triangulate_counts* counts, int32_t* n_matches, int32_t* n_created);
/* per slot, n_neighbours x n_keypoints entries each (xyz three floats per slot); any may be NULL */
iba_status iba_triangulation_read(const iba_triangulation* t, int32_t job, uint8_t* status, int32_t* match, int32_t* dist, float* xyz);
/* R8: the job's n_created points in creation order; any may be NULL */
iba_status iba_triangulation_points(const iba_triangulation* t, int32_t job, int32_t* idx1, int32_t* neighbour, int32_t* idx2, float* xyz /* x 3 */, float* normal /* x 3 */,
                                    float* min_dist, float* max_dist, uint8_t* desc /* x 32 */);
/* keep_stages only: per slot the length of its candidate segment (0 where the slot ended in R1 or R2) */
iba_status iba_triangulation_segments(const iba_triangulation* t, int32_t job, int32_t* seg_len);
/* host only, pure: KeyFrame::ComputeSceneMedianDepth(q) over n world points */
iba_status iba_triangulate_median_depth(const float* Tcw12, const float* xyz /* n x 3 */, int32_t n, int32_t q, float* out);

/*
 * ---- Map-point fusion [the camera side's eighth brick: the reference's LocalMapping::SearchInNeighbors (src/orb_slam/src/LocalMapping.cc:453-533)
 * with ORBmatcher::Fuse(KeyFrame*, const vector<MapPoint*>&, th) (ORBmatcher.cc:825-975), its Sim3 overload's loop (:977-1100) and
 * MapPoint::Replace (MapPoint.cc:190-228)] ----
 * The step that keeps the map from growing duplicates: the points of the current keyframe are projected into the target keyframes and the
 * targets' points back into the current one; a point that lands on a keypoint which already holds a point is merged with it, one that lands on a
 * free keypoint becomes an observation. A call takes F frames (iba_orb_frame; xy is mvKeysUn), ONE table of P map points (iba_map_points) and J
 * jobs; a job is one Fuse call: a keyframe (frame, pose, intrinsics, tables) and a list of points. Frames and the table go up once, however many
 * jobs name them. TWO FACTS OF THE REFERENCE split the work. (1) Inside one Fuse call the projection, the gates, the predicted level, the window
 * and the best keypoint (bestIdx, bestDist) of a listed point depend only on the point and the keyframe, never on what earlier points of the list
 * did: isBad() and IsInKeyFrame(pKF) only skip a point. So every (job, list position) slot is independent: iba_fuse, on the device. (2) What is
 * done with a pick - AddObservation, or Replace in one of two directions by Observations() - reads and changes the map graph and is sequential:
 * iba_fuse_apply, a host fold over the caller's map arrays, O(number of picks). JOBS ARE INDEPENDENT and use the point table as given.
 * Float arithmetic is float32 unless a cast says otherwise, every operation rounded, evaluated left to right, no contraction;
 * tests/fuse_ref.py restates the device rules in numpy, sequentially as the reference is written, and the fold as MapPoint / KeyFrame objects; the
 * device and the host restatement (iba_debug_fuse_host) are compared with it byte for byte. The float decisions are ONE text, csrc/iba_fuse_math.hpp,
 * which reuses csrc/iba_map_match_math.hpp wherever a rule is literally L1's.
 *
 *   F1 skip.       Per listed point, in list order. A list entry < 0 (the reference's NULL pointer) or a set skip byte (isBad() ||
 *                  IsInKeyFrame(pKF) at call time; iba_fuse_skip computes it) gives SKIPPED. The point is not projected.
 *   F2 projection. Pc as in L1, the same order of sums. PcZ < 0.0f: DEPTH. invz = (float)(1.0 / (double)PcZ). x = PcX * invz, y = PcY * invz,
 *                  u = fx * x + cx, v = fy * y + cy: Fuse's association, which differs from L1's (fx * PcX) * invz. u or v not finite:
 *                  NOT_FINITE (the reference skips such a point too, IsInImage is false for NaN and infinity; only the status name is the
 *                  library's). KeyFrame::IsInImage is HALF OPEN: u >= min_x && u < max_x && v >= min_y && v < max_y, anything else BOUNDS: a
 *                  centre exactly on max_x is refused here, where L1 keeps it.
 *   F3 distance and angle. Ow, PO and dist are L1's. dist < 0.8f * min_dist || dist > 1.2f * max_dist: DISTANCE (exactly on a bound is kept).
 *                  dot = (PO_0 n_0 + PO_1 n_1) + PO_2 n_2 in double; dot < (double)view_cos_limit * (double)dist: ANGLE. No division: this is
 *                  Fuse's form (PO.dot(Pn) < 0.5 * dist3D), not L1's view_cos.
 *   F4 level and window. ratio = max_dist / dist (float32, correctly rounded) and the level by L1's table rule. radius = th *
 *                  scale_factors[level]. The list is M3's with centre (u, v), that radius and levels (level - 1, level), the distances M4's
 *                  against the point's descriptor. This equals KeyFrame::GetFeaturesInArea(u, v, r) followed by Fuse's kpLevel test, in the same
 *                  order, because the test only deletes entries of the list. An empty list: NO_CANDIDATE.
 *   F5 pick.       A candidate is ELIGIBLE iff its distance is below 256 and it passes the gate. The gate applies only where
 *                  check_reprojection is set: ex = u - kp_x, ey = v - kp_y, e2 = ex * ex + ey * ey; the candidate passes iff NOT
 *                  (double)(e2 * inv_level_sigma2[octave]) > (double)chi2_mono (the reference's 5.99 is a double literal). The pick is the
 *                  lexicographic minimum of (distance, list position) over the eligible candidates; the device reduces the key
 *                  (distance << 32) | position. PICKED iff a pick exists and its distance <= th_low; otherwise NO_MATCH.
 *                  WHY THE MINIMUM IS THE REFERENCE'S WALK. The reference starts (bestDist, bestIdx) at (256, -1) and walks the list with
 *                  `if (dist < bestDist) take it`, skipping the candidates the gate refuses. Invariant: after any prefix, (bestDist, bestIdx) is
 *                  the least (distance, position) pair among the prefix's eligible candidates, or (256, -1). A new eligible candidate has the
 *                  largest position so far: it is the new least pair iff its distance is strictly below bestDist; at 256 or above it never is.
 *                  With check_reprojection == 0 this is the loop of the Sim3 overload, which starts bestDist at INT_MAX: that changes no PICKED
 *                  outcome for th_low < 256, because only a candidate at 256 is treated differently and it is never <= th_low; the caller
 *                  passes Rcw = sRcw / s, tcw = t / s in Tcw12.
 *   F6 outputs per job. Per listed point: status (uint8), u, v, level, radius (zeros where F4 was not reached), match (the keypoint, -1 unless
 *                  PICKED) and dist (the pick's distance, -1 unless PICKED). Counts: one per status, n_candidates (the sum of the list lengths),
 *                  n_picked. With keep_stages the candidate lists in M3's order as iba_map_matches_lists gives them.
 *
 * THE FOLD (iba_fuse_apply, host only, pure). The state is the caller's map (iba_fuse_map), changed IN PLACE.
 *   U1 state.      IsInKeyFrame(p, k) holds iff some keypoint of keyframe k holds p. Observations(p) = the number of keyframes that hold p (the
 *                  monocular nObs). THE MAP MUST NAME EVERY KEYFRAME THAT OBSERVES AN INVOLVED POINT: what it does not name does not exist for
 *                  the fold. Refused at entry with IBA_ERR_INVALID_ARG: a point held twice in one keyframe, a holder entry outside [-1, P), a
 *                  keyframe whose keypoint count differs from the job's frame. The point -> (keyframe, keypoint) index is built once per call.
 *   U2 order.      The job's list positions in order; only PICKED entries act (every other op is NONE). A PICKED entry whose point is bad by
 *                  now: STALE_BAD; one whose point is by now held in the keyframe: STALE_IN_KEYFRAME. Both are the reference's `continue`,
 *                  reached through an earlier fold or a duplicated list entry; neither counts as fused.
 *   U3 act.        q = holder[keyframe][match]. q < 0: ADD, holder[keyframe][match] = p. q >= 0 && bad[q]: HELD_BAD, no change. Otherwise in
 *                  LOCAL mode: Observations(q) > Observations(p): p dies into q (REPLACED_BY_HELD), else q dies into p (REPLACES_HELD; equality
 *                  takes this branch, as the reference's `>` dictates); in LOOP mode: RECORD, no change (vpReplacePoint[match] = p). other = q in
 *                  every case but ADD. All of these count in n_fused, as the reference counts them.
 *   U4 Replace(a dies, b survives). For every (k', i) that holds a: where b is held in k', holder[k'][i] = -1, otherwise holder[k'][i] = b.
 *                  bad[a] = 1, replaced_by[a] = b, found[b] += found[a], visible[b] += visible[a], descriptor_stale[b] = 1 (the last three where
 *                  the arrays are given). Each step depends only on (a, b, k'), so the order over the keyframes changes no outcome.
 *   U5 helpers.    iba_fuse_skip: F1's bytes from the map (entry < 0, bad, or held in the keyframe). iba_fuse_candidates: vpFuseCandidates -
 *                  the targets in order, their keypoints in ascending index, each held point that is not bad and not already listed.
 *
 * UNPINNED, as in L1: the order of the sums of Pc, Ow, the dot product and cv::norm. KNOWN DEVIATIONS: (1) the level by the table rule in place of
 * libm's ceil(log(ratio) / mfLogScaleFactor), as in L1. (2) NO DESCRIPTOR REFRESH: Replace ends with ComputeDistinctiveDescriptors() on the
 * survivor, so in the reference a survivor enters the next target keyframe with a new descriptor; every job of a call uses the table as given and
 * the fold marks the survivors (descriptor_stale) for the caller or a later brick (profiles/fuse_parity.md counts how often the refresh would have
 * changed a pick). (3) NOT_FINITE, a name only.
 * NOT PROVIDED: stereo (mvuRight, ur, the 7.8 gate), the choice of target keyframes (covisibility), UpdateConnections. The "Update points" tail
 * of SearchInNeighbors and the refresh inside Replace are iba_refresh (below): iba_fuse_apply, iba_refresh_observations, iba_refresh of the
 * descriptor_stale survivors, iba_refresh_store.
 * DEVICE (csrc/iba_fuse_kernels.hpp). Before the chunks, over the whole call: the frustum kernel - a flat table of (job, list position) slots, one
 * lane per slot, blocks that do not straddle a job so that pose, intrinsics, bounds and tables are uniform per block; F1-F4; it writes the status
 * and the slot's query record and counts the statuses by wave ballot into LDS with one integer atomic per counter and block; then the matcher's
 * grid kernels and its list kernel, unchanged - the point descriptors lie behind the keypoint descriptors in the one flat descriptor table, as in
 * iba_map_match. Per chunk of consecutive jobs: scan, the list kernel writing candidates and distances, and the pick kernel: W lanes per slot (W =
 * 8, 16 or 64; 8 ships, profiles/fuse_bench.md), the lanes stride over the slot's segment of (candidate, distance) entries, gather the candidate's
 * position and octave for the gate, keep their least key; the group minimum by xor shuffles inside the aligned group; one lane writes match, dist
 * and status; the NO_CANDIDATE / NO_MATCH / PICKED counts go the way of the frustum's. No floating-point atomics, and no byte depends on the
 * arrival order of an atomic.
 * MEMORY: the candidate lists (IBA_FUSE_BYTES_PER_CANDIDATE bytes per entry, sized from the count pass) are cut into chunks of consecutive jobs
 * under IBA_FUSE_BUDGET_BYTES, or under a quarter of the device memory free at the call where that is less; a chunk holds at least one job and a
 * chunk boundary changes no byte. A chunk whose lists hold 2^31 entries or more answers IBA_ERR_UNSUPPORTED. The result is host memory and keeps
 * a copy of every job's list, because the fold needs it.
 * ERRORS, all IBA_ERR_INVALID_ARG with a message (iba_fuse_last_error, per thread) BEFORE the device is touched: a NULL argument (the table's
 * arrays may be NULL only where P == 0; skip may always be NULL; points may be NULL only where n_points == P: all P in order) or a wrong
 * struct_size; J < 1, F < 1, P < 0; a frame that iba_orb_match would refuse; a job's frame out of range or a listed point >= P; n_points < 0; a
 * pose entry, point, normal, distance, intrinsic or th that is not finite or whose magnitude is above 1e6; n_levels outside [1,
 * IBA_MAP_MATCH_MAX_LEVELS]; a scale table that is not finite, does not start at 1 or does not ascend strictly; an inv_level_sigma2 that is not
 * finite, above 1e6 or <= 0; an octave of the job's frame outside [0, n_levels); th_low outside [0, 256]; view_cos_limit or chi2_mono not finite;
 * a job index outside the result; the stage accessor on a result without keep_stages; the fold's U1 checks, a keyframe outside the map, a mode
 * that is neither, a listed point >= the map's P. A job with n_points == 0 and a frame with n == 0 are legal.
 */
#define IBA_FUSE_BUDGET_BYTES (1ull << 30)
#define IBA_FUSE_BYTES_PER_CANDIDATE 6ull
#define IBA_FUSE_N_STATUS 9
typedef enum iba_fuse_status {
    IBA_FUSE_PICKED = 0, IBA_FUSE_SKIPPED = 1, IBA_FUSE_DEPTH = 2, IBA_FUSE_NOT_FINITE = 3, IBA_FUSE_BOUNDS = 4, IBA_FUSE_DISTANCE = 5, IBA_FUSE_ANGLE = 6,
    IBA_FUSE_NO_CANDIDATE = 7, IBA_FUSE_NO_MATCH = 8
} iba_fuse_status;
typedef struct iba_fuse_job {                 /* host pointers, read during the call only */
    int32_t frame;                  /* index into the call's frame array */
    int32_t n_levels;               /* entries of scale_factors and inv_level_sigma2, 1..IBA_MAP_MATCH_MAX_LEVELS */
    int32_t n_points;
    float   th;                     /* 3.0f */
    float   fx, fy, cx, cy;
    const float*   Tcw12;           /* 3 x 4 row-major float32: the keyframe's pose */
    const float*   scale_factors;   /* n_levels: mvScaleFactors, [0] == 1, ascending */
    const float*   inv_level_sigma2;/* n_levels: mvInvLevelSigma2 */
    const int32_t* points;          /* n_points table indices in list order; an entry < 0 is the reference's NULL pointer; NULL: all P in order */
    const uint8_t* skip;            /* n_points, or NULL: none: isBad() || IsInKeyFrame(pKF) at call time */
} iba_fuse_job;
typedef struct iba_fuse_options {
    int32_t struct_size;        /* sizeof(iba_fuse_options) */
    int32_t th_low;             /* 50 */
    float   view_cos_limit;     /* 0.5f, widened (F3) */
    float   chi2_mono;          /* 5.99f, widened (F5) */
    int32_t check_reprojection; /* 1; 0: the Sim3 overload's loop */
    int32_t keep_stages;        /* 0; 1 keeps the candidate lists for iba_fusion_lists */
} iba_fuse_options;
typedef struct iba_fuse_counts {
    int32_t n_points;
    int32_t status[IBA_FUSE_N_STATUS];   /* by iba_fuse_status */
    int32_t n_candidates, n_picked;      /* n_picked = status[IBA_FUSE_PICKED] */
} iba_fuse_counts;
typedef struct iba_fusion iba_fusion;
iba_status iba_default_fuse_options(iba_fuse_options* opt);
const char* iba_fuse_last_error(void);                               /* never NULL; of this thread's last iba_fus* call that failed */
/* *out is NULL on failure; release it with iba_fusion_free */
iba_status iba_fuse(const iba_orb_frame* frames, int32_t F, const iba_map_points* points, const iba_fuse_job* jobs, int32_t J, const iba_fuse_options* opt, int device,
                    iba_fusion** out);
void       iba_fusion_free(iba_fusion* f);
int32_t    iba_fusion_n_jobs(const iba_fusion* f);                   /* 0 for NULL */
iba_status iba_fusion_job(const iba_fusion* f, int32_t job, iba_fuse_counts* counts);
/* F6 per listed point, n_points entries each; any may be NULL */
iba_status iba_fusion_read(const iba_fusion* f, int32_t job, uint8_t* status, float* u, float* v, int32_t* level, float* radius, int32_t* match, int32_t* dist);
/* keep_stages only: off[n_points + 1] and, per entry, the keypoint and the distance in M3's order; their length is the job's n_candidates. Every
 * output may be NULL. */
iba_status iba_fusion_lists(const iba_fusion* f, int32_t job, int32_t* off, int32_t* index, uint16_t* dist);

/* the fold (U1-U5): host only, pure */
#define IBA_FUSE_LOCAL 0        /* Fuse(pKF, vpMapPoints, th): Replace by Observations() */
#define IBA_FUSE_LOOP  1        /* the Sim3 overload: record vpReplacePoint, change nothing */
typedef enum iba_fuse_op {
    IBA_FUSE_OP_NONE = 0, IBA_FUSE_OP_ADD = 1, IBA_FUSE_OP_REPLACED_BY_HELD = 2, IBA_FUSE_OP_REPLACES_HELD = 3, IBA_FUSE_OP_HELD_BAD = 4, IBA_FUSE_OP_RECORD = 5,
    IBA_FUSE_OP_STALE_BAD = 6, IBA_FUSE_OP_STALE_IN_KEYFRAME = 7
} iba_fuse_op;
typedef struct iba_fuse_map {
    int32_t K;                  /* the keyframes of the map */
    const int32_t* kp_off;      /* K + 1: keyframe k's keypoints are holder[kp_off[k] .. kp_off[k + 1]) */
    int32_t* holder;            /* kp_off[K]: mvpMapPoints of every keyframe of the map, a table index or -1 */
    int32_t P;
    uint8_t* bad;               /* P */
    int32_t* replaced_by;       /* P, -1: mpReplaced */
    int32_t* found;             /* P, may be NULL */
    int32_t* visible;           /* P, may be NULL */
    uint8_t* descriptor_stale;  /* P, may be NULL: set on every survivor of a Replace */
} iba_fuse_map;
/* the fold of one job of f into the map; keyframe = the job's pKF in the map. op and other take n_points entries each (other: the held point, or
 * -1) and may be NULL, as may n_fused (the reference's return value) */
iba_status iba_fuse_apply(const iba_fusion* f, int32_t job, int32_t keyframe, iba_fuse_map* map, int32_t mode, int32_t* op, int32_t* other, int32_t* n_fused);
/* U5: F1's bytes for a list against a keyframe of the map */
iba_status iba_fuse_skip(const iba_fuse_map* map, int32_t keyframe, const int32_t* points, int32_t n, uint8_t* skip);
/* U5: vpFuseCandidates over T target keyframes; points takes up to map->P entries, *n is their number */
iba_status iba_fuse_candidates(const iba_fuse_map* map, const int32_t* targets, int32_t T, int32_t* points, int32_t* n);

/*
 * ---- Map-point refresh [the camera side's ninth brick: the reference's MapPoint::ComputeDistinctiveDescriptors (src/orb_slam/src/MapPoint.cc:255-320)
 * and MapPoint::UpdateNormalAndDepth (:343-384), the two functions it calls most often on the map: after CreateNewMapPoints, at the end of
 * MapPoint::Replace, in the "Update points" tail of SearchInNeighbors (LocalMapping.cc:515-530) and after every bundle adjustment] ----
 * For a batch of map points in ONE call: the representative descriptor (the observed descriptor with the least median Hamming distance to the
 * others), the mean viewing direction and the two scale-invariance distances, from the points' observations. It closes the loop of one
 * LocalMapping step inside the C ABI: iba_triangulate / iba_fuse + iba_fuse_apply / iba_bundle_optimize change the map, iba_refresh brings normal,
 * min_dist, max_dist and desc of the iba_map_points table up to date, iba_refresh_store writes them back, and the next iba_map_match / iba_fuse
 * reads a table that is not stale. A call takes F frames (iba_orb_frame: ONLY desc, octave and n are read), K keyframes (iba_refresh_keyframe:
 * the frame, the pose, the scale table, isBad()), ONE table of P points, read as given, point_bad[P] (MapPoint::isBad(); may be NULL: none),
 * ref_keyframe[P] (mpRefKF as a keyframe index) and the observations of every point as CSR lists: obs_off[P + 1], obs_keyframe[], obs_keypoint[].
 * THE ORDER INSIDE A POINT'S LIST IS THE CALLER'S AND IS PART OF THE RULE: the reference iterates a std::map<KeyFrame*, size_t>, that is in
 * pointer order, which nothing can pin (iba_triangulate's deviation (2) says the same). list[n] names the points to refresh in output order
 * (NULL: all P in order, and n must be P); a duplicated entry is legal and gives equal results. Every point is independent of every other.
 * Integer work is exact. Float arithmetic is float32 unless a cast says otherwise, every operation rounded, left to right, no contraction, as in
 * L1 / R8; tests/refresh_ref.py restates the rules in numpy as the reference is written (the full matrix, a sort of every row, the `<` walk); the
 * device and the host restatement (iba_debug_refresh_host) are compared with it byte for byte. The decisions are ONE text, csrc/iba_refresh_math.hpp.
 *
 *   S1 select.     point_bad set: BAD. An empty observation list: EMPTY. Both are the reference's early returns; all four outputs are the table's
 *                  values as given, desc_state and geo_state NONE, best_obs = best_median = -1, n_desc = 0.
 *   S2 descriptor set. The observations whose keyframe is not bad, in list order: N of them; entry i is desc row obs_keypoint of the keyframe's
 *                  frame. N == 0: desc_state KEPT, the descriptor as given, best_obs = best_median = -1; S4 and S5 still run, because
 *                  UpdateNormalAndDepth never looks at isBad(). Otherwise desc_state PICKED.
 *   S3 median pick. d(i, j) is the 256-bit Hamming distance, d(i, i) = 0. m = (N - 1) / 2 in integer division: the reference's
 *                  vDists[0.5 * (N - 1)], truncated. median(i) is the element of rank m of row i in ascending order; equivalently THE LEAST v SUCH
 *                  THAT AT LEAST m + 1 ENTRIES OF ROW i ARE <= v, which is the form the device and the host restatement evaluate (no sort). The
 *                  pick is the lexicographic minimum of (median(i), i); the device reduces the key (median << 32) | i.
 *                  WHY THE MINIMUM IS THE REFERENCE'S WALK. The reference starts BestMedian at INT_MAX and walks the rows in order with
 *                  `if (median < BestMedian) take it`. Invariant: after any prefix of rows, (BestMedian, BestIdx) is the least (median, row) pair
 *                  of the prefix. The next row has the largest index so far: it is the new least pair iff its median is strictly below
 *                  BestMedian; at a tie the earlier row holds. A median is at most 256 < INT_MAX, so row 0 is always taken. And the rank form
 *                  equals the sorted element: the sorted row's entry m is the least value with at least m + 1 entries at or below it.
 *                  best_obs is the picked row's position in the point's FULL observation list, best_median its median, n_desc = N.
 *   S4 normal.     Ow of a keyframe is L1's formula, formed once per keyframe. Per observation k of the FULL list, in order: PO = P - Ow_k
 *                  (float32), |PO| = L1's dist before its narrowing (squares and sums in double), term_c = (float)((double)PO_c / |PO|): exactly
 *                  R8's n_i. sum_c starts at 0.0f and adds the terms in float32 IN LIST ORDER. normal_c = (float)((double)sum_c / (double)n), n
 *                  the length of the full list. For n == 2 this is R8's (n1 + n2) * 0.5f bit for bit.
 *   S5 distances.  The reference keyframe's entry is the first one of the list whose keyframe equals ref_keyframe. dist = (float)|P - Ow_ref|,
 *                  level = the octave of that entry's keypoint, max_dist = dist * scale_factors_ref[level], min_dist = max_dist /
 *                  scale_factors_ref[n_levels_ref - 1], correctly rounded (R8's). geo_state UPDATED.
 *   S6 guards.     The library's own. ref_keyframe not in the list: geo_state NO_REF, the normal computed, the distances as given. Any |PO| == 0:
 *                  geo_state DEGENERATE, normal and distances as given.
 *   S7 outputs per listed point. status (REFRESHED / BAD / EMPTY), desc_state, geo_state (uint8 each), best_obs, best_median, n_desc, normal,
 *                  min_dist, max_dist, desc. Counts of the call: one per status and state, n_desc_changed (PICKED and the picked 32 bytes differ
 *                  from the table's), path[3] (the points on each device shape; zeros from the host restatement) and n_rows. With keep_stages:
 *                  per REFRESHED point the median of every observation's row in the order of the FULL list, -1 for an observation of a bad
 *                  keyframe (iba_refreshed_medians; n_rows entries).
 *
 * HELPERS, host only, pure. iba_refresh_observations builds the CSR lists from an iba_fuse_map: keyframes in ascending index, each (keyframe,
 * keypoint) that holds p once, so that the output of iba_fuse_apply feeds the refresh; a point held twice in one keyframe is refused as in U1.
 * iba_refresh_store scatters the REFRESHED entries of a result into the caller's MUTABLE table arrays by listed index and clears
 * descriptor_stale there where the array is given.
 * UNPINNED, as in L1: the order of the sums of Ow and cv::norm. KNOWN DEVIATIONS: (1) the list order in place of pointer order, above
 * (profiles/refresh_parity.md counts what the order can change). (2) NO_REF: the reference's observations[pRefKF] on its local copy would insert
 * 0 and read keypoint 0. (3) DEGENERATE: the reference divides by zero.
 * NOT PROVIDED: stereo, UpdateConnections, culling, and the refresh between the jobs of one iba_fuse call (iba_fuse is unchanged).
 * DEVICE (csrc/iba_refresh_kernels.hpp). The host, which holds obs_off, settles S1 and bins the other listed points by the length of their FULL
 * list into three work lists; ONE kernel text runs in three shapes, a group of G lanes per point: NARROW (G = 4, 8, 16 or 32 for lists of up to G
 * entries, 256 / G points per block; 16 ships, profiles/refresh_bench.md), WAVE (G = 64: one wave per point, lane i owns row i) and BLOCK (G = 256:
 * one block per point, up to IBA_REFRESH_MAX_OBS entries, rows strided over the threads). The group gathers descriptor (32 bytes), S4's term and
 * keyframe of every observation into LDS once (32 KiB of descriptors at the cap); a lane holds its own row's descriptor in four 64-bit registers
 * and reads descriptor j at an address uniform across the group, an LDS broadcast; d(i, j) is four xor + popcount. NO N x N TABLE GOES TO GLOBAL
 * MEMORY: the call allocates inputs and outputs only, so there is no budget and no chunking. The median of a row is S3's counting form, either a
 * 9-step binary search on v that recomputes the row's distances at every step, or one pass that keeps the row - in LDS for the narrow and wave
 * shapes, in the registers of a wave that takes the row for the block shape - and searches there (ships; profiles/refresh_bench.md records both). The
 * pick is the group minimum of the key by xor shuffles (and 4 LDS words for the block). S4 / S5 run in the same kernel: the lanes stride over the
 * full list for the terms, then lane 0 adds them in list order, because the order is the rule. No floating-point atomics, and no byte depends on
 * the arrival order of an atomic: the counts go by ballot into LDS and one integer atomic per counter and block.
 * ERRORS, all IBA_ERR_INVALID_ARG with a message (iba_refresh_last_error, per thread) BEFORE the device is touched: a NULL argument (point_bad and
 * list may be NULL; the table's arrays and ref_keyframe only where P == 0; obs_keyframe and obs_keypoint only where obs_off[P] == 0) or a wrong
 * struct_size; F < 1, K < 1, P < 0, n < 0; list NULL and n != P; a frame that iba_orb_match would refuse; a keyframe's frame out of range; a pose
 * entry, point, normal or distance that is not finite or whose magnitude is above 1e6; n_levels outside [1, IBA_REFRESH_MAX_LEVELS]; a scale table
 * that is not finite, does not start at 1 or does not ascend strictly; obs_off not ascending from 0; an observation's keyframe or keypoint out of
 * range; one keyframe twice in a point's list (a std::map cannot hold that); an octave of an observed keypoint outside [0, n_levels) of its
 * keyframe; a listed point, or the ref_keyframe of a listed point, outside its range; the stage accessor on a result without keep_stages. A listed
 * point with more than IBA_REFRESH_MAX_OBS observations, or 2^31 observations or keypoints in a call, answer IBA_ERR_UNSUPPORTED.
 */
/* 1024: a block's LDS holds the descriptors (32 KiB), terms and keyframes of one point. The reference's own `int Distances[N][N]` on the stack is
 * 4 MiB there and passes the default 8 MiB stack at N = 1449. */
#define IBA_REFRESH_MAX_OBS 1024
#define IBA_REFRESH_MAX_LEVELS 64
typedef enum iba_refresh_status { IBA_REFRESH_REFRESHED = 0, IBA_REFRESH_BAD = 1, IBA_REFRESH_EMPTY = 2 } iba_refresh_status;
typedef enum iba_refresh_desc_state { IBA_REFRESH_DESC_NONE = 0, IBA_REFRESH_DESC_PICKED = 1, IBA_REFRESH_DESC_KEPT = 2 } iba_refresh_desc_state;
typedef enum iba_refresh_geo_state {
    IBA_REFRESH_GEO_NONE = 0, IBA_REFRESH_GEO_UPDATED = 1, IBA_REFRESH_GEO_NO_REF = 2, IBA_REFRESH_GEO_DEGENERATE = 3
} iba_refresh_geo_state;
typedef enum iba_refresh_path { IBA_REFRESH_PATH_NARROW = 0, IBA_REFRESH_PATH_WAVE = 1, IBA_REFRESH_PATH_BLOCK = 2 } iba_refresh_path;
typedef struct iba_refresh_keyframe {         /* host pointers, read during the call only */
    int32_t frame;                  /* index into the call's frame array */
    int32_t n_levels;               /* entries of scale_factors, 1..IBA_REFRESH_MAX_LEVELS */
    const float* Tcw12;             /* 3 x 4 row-major float32: the keyframe's pose */
    const float* scale_factors;     /* n_levels: mvScaleFactors, [0] == 1, ascending */
    int32_t bad;                    /* KeyFrame::isBad() */
    int32_t reserved;               /* 0 */
} iba_refresh_keyframe;
typedef struct iba_refresh_options {
    int32_t struct_size;        /* sizeof(iba_refresh_options) */
    int32_t keep_stages;        /* 0; 1 keeps the median of every row for iba_refreshed_medians */
} iba_refresh_options;
typedef struct iba_refresh_counts {
    int32_t n_points;
    int32_t status[3];          /* by iba_refresh_status */
    int32_t desc_state[3];      /* by iba_refresh_desc_state */
    int32_t geo_state[4];       /* by iba_refresh_geo_state */
    int32_t n_desc_changed;
    int32_t path[3];            /* by iba_refresh_path: the points each device shape took */
    int32_t n_rows;             /* keep_stages: the entries of iba_refreshed_medians */
} iba_refresh_counts;
typedef struct iba_refreshed iba_refreshed;
iba_status iba_default_refresh_options(iba_refresh_options* opt);
const char* iba_refresh_last_error(void);                            /* never NULL; of this thread's last iba_refresh* call that failed */
/* *out is NULL on failure; release it with iba_refreshed_free */
iba_status iba_refresh(const iba_orb_frame* frames, int32_t F, const iba_refresh_keyframe* keyframes, int32_t K, const iba_map_points* points, const uint8_t* point_bad,
                       const int32_t* ref_keyframe, const int32_t* obs_off, const int32_t* obs_keyframe, const int32_t* obs_keypoint, const int32_t* list, int32_t n,
                       const iba_refresh_options* opt, int device, iba_refreshed** out);
void       iba_refreshed_free(iba_refreshed* r);
int32_t    iba_refreshed_n(const iba_refreshed* r);                  /* the listed points; 0 for NULL */
iba_status iba_refreshed_counts(const iba_refreshed* r, iba_refresh_counts* counts);
/* S7 per listed point, n entries each (normal n x 3, desc n x 32); any may be NULL */
iba_status iba_refreshed_read(const iba_refreshed* r, uint8_t* status, uint8_t* desc_state, uint8_t* geo_state, int32_t* best_obs, int32_t* best_median, int32_t* n_desc, float* normal,
                              float* min_dist, float* max_dist, uint8_t* desc);
/* keep_stages only: off[n + 1] and the medians (n_rows entries); either may be NULL */
iba_status iba_refreshed_medians(const iba_refreshed* r, int32_t* off, int32_t* median);
/* host only, pure: obs_off takes map->P + 1 entries, obs_keyframe and obs_keypoint up to map->kp_off[map->K] each (obs_off[P] are written) */
iba_status iba_refresh_observations(const iba_fuse_map* map, int32_t* obs_off, int32_t* obs_keyframe, int32_t* obs_keypoint);
/* host only, pure: the REFRESHED entries of r into the table's arrays of P points (normal P x 3, desc P x 32); descriptor_stale may be NULL */
iba_status iba_refresh_store(const iba_refreshed* r, int32_t P, float* normal, float* min_dist, float* max_dist, uint8_t* desc, uint8_t* descriptor_stale);

/*
 * ---- Sim3 RANSAC between two keyframes [the camera side's tenth brick and the first of LoopClosing: the reference's Sim3Solver
 * (src/orb_slam/src/Sim3Solver.cc), driven from LoopClosing::ComputeSim3 (LoopClosing.cc:231-342)] ----
 * For J keyframe pairs in ONE call: a RANSAC over 3-point sets of matched map points. Horn's closed-form absolute orientation gives each
 * hypothesis, every hypothesis is scored by reprojecting every correspondence both ways, and a sequential best / early-return rule picks the result.
 * It is the only monocular step that recovers the scale drift around a loop. A call takes ONE table of P map points (iba_map_points: ONLY xyz and n
 * are read) and J jobs; a job is the two keyframes' poses and intrinsics, n correspondences as table indices (point1 seen from keyframe 1, point2
 * from keyframe 2), their thresholds and the 3-point sets. The iterations of a job are Z6's budget, computed by the call from n and the options; the
 * job's sets hold max_iterations rows, of which the first `iterations` are read. Every iteration of every job is computed, whatever the events: the
 * host has nothing to do between upload and download, and iba_sim3_iterate replays the reference's iterate(n) calls over the finished result.
 * ARITHMETIC as in the two-view unit: float32 wherever the reference holds a float; every cv::Mat operation in float64 on the widened entries with
 * ONE rounding per result element, sums left to right; no contraction. tests/sim3_ref.py restates every rule in numpy, sequentially as the reference
 * runs; the device and the host restatement (iba_debug_sim3_host) are compared with it byte for byte. The float decisions are ONE text,
 * csrc/iba_sim3_math.hpp.
 *
 *   Z1 thresholds. mvnMaxError is a vector<size_t>: the bound is (size_t)(9.210 * (double)sigma2), TRUNCATED (13 for 1.44f, not 13.26), and is
 *                  compared as a float32 with err < bound. iba_sim3_correspondences writes that truncated value into max_err1 / max_err2; the device
 *                  compares with max_err as given.
 *   Z2 preparation. Per correspondence and camera: Xc_i = ((R_i0 X + R_i1 Y) + R_i2 Z) + t_i in float32, L1's order of sums. The image point
 *                  (FromCameraToImage): invz = 1 / z in float32, correctly rounded, formed as (float)(1.0 / (double)z); u = fx * (x * invz) + cx,
 *                  v = fy * (y * invz) + cy. There is NO test on z: a point at or behind the camera gives inf or NaN, which flow through as in the
 *                  reference.
 *   Z3 Horn.       (:226-337) P1, P2: the set's three points in camera 1 / 2 as columns. Per row the sum ((a + b) + c) in double, rounded; the
 *                  centroid O = that sum / 3 in double, rounded; Pr = P - O. M = Pr2 Pr1^T, entry (i, j) = (float)(sum over k of Pr2_ik Pr1_jk).
 *                  The ten entries of N in double from M's float32 entries, left to right as the reference writes them (N11 = (M00 + M11) + M22,
 *                  N33 = (-M00 + M11) - M22, ...), stored as float32. The eigenvector of the greatest eigenvalue: a cyclic two-sided Jacobi in
 *                  float64 on the widened 4 x 4, V = I; the pairs (p, q) in the order (0,1) (0,2) (0,3) (1,2) (1,3) (2,3); a pair with |a_pq| <=
 *                  2^-53 (|a_pp| + |a_qq|) is left alone; else theta = (a_qq - a_pp) / (2 a_pq), t = sign(theta) / (|theta| + sqrt(1 + theta^2))
 *                  with sign(0) = +1, c = 1 / sqrt(1 + t^2), s = c t; columns p, q of A and V become (c x_p - s x_q, s x_p + c x_q), then rows
 *                  p, q of A likewise, then a_pq = a_qp = 0 exactly. A sweep without a rotation ends it; the cap is 30 sweeps. The eigenvalue
 *                  is the greatest diagonal entry, the FIRST on a tie; its column of V narrowed to float32 is the quaternion (w, x, y, z).
 *                  R is Z4's. P3 = R Pr2 (float32 entries of double sums); nom = the double sum over (i, j) in row-major order of Pr1_ij P3_ij;
 *                  den = the double sum in the same order of the float32 squares P3_ij * P3_ij; s = (float)(nom / den), or 1.0f with fix_scale.
 *                  sR = s R (float32); t = O1 - sR O2; T12 = [sR | t]; T21 = [Ri | -(Ri t)] with Ri_ij = (float)((1.0 / (double)s) * R_ji).
 *   Z4 rotation.   R from the quaternion directly, in float64 with one rounding per entry: n = ((w^2 + x^2) + y^2) + z^2, R00 = 1 - 2 (y^2 + z^2) / n,
 *                  R01 = 2 (x y - w z) / n, R02 = 2 (x z + w y) / n, R10 = 2 (x y + w z) / n, R11 = 1 - 2 (x^2 + z^2) / n, R12 = 2 (y z - w x) / n,
 *                  R20 = 2 (x z - w y) / n, R21 = 2 (y z + w x) / n, R22 = 1 - 2 (x^2 + y^2) / n. Where sqrt((x^2 + y^2) + z^2) is 0 or not finite
 *                  the reference divides by it: every entry of s, R, t, T12, T21 is then NaN and the hypothesis has 0 inliers.
 *   Z5 score.      (:340-364) Project: p = T X as a matrix product (one rounding) plus the translation (float32), then the image point as in
 *                  Z2. err1 from camera 2's point through T12 and K1 against camera 1's image point, err2 the other way: d = the float32
 *                  differences, err = (float)(d_0^2 + d_1^2) in double. Inlier iff err1 < max_err1 && err2 < max_err2; a NaN never passes.
 *   Z6 budget.     (:114-138, host only) eps = (float)min_inliers / N in float32. N == min_inliers: 1 iteration. Else
 *                  ceil(log(1 - probability) / log(1 - pow((double)eps, 3))) clamped to [1, max_iterations]; where the quotient is not finite the
 *                  library's own rule is max_iterations. log and pow are the host's libm.
 *   Z7 the sequential rule. (:158-206) best = 0; the iterations in order; iteration `it` with n inliers REPLACES THE BEST iff n >= best: ties go to
 *                  the LATER iteration, and an iteration with 0 inliers replaces a best of 0. It is an EVENT iff it also has n > min_inliers:
 *                  an event is where the reference's iterate returns. The scan does not stop at an event: a caller whose optimiser refuses the
 *                  result calls iterate again with the best retained. Hence events are numbered; the first max_events of a job are listed with
 *                  their inlier bytes.
 *   Z8 status.     OK: at least one event; the reference's find() is event 0. NO_MORE: no event within the budget. TOO_FEW: N < min_inliers
 *                  (bNoMore at :146), decided on the host; such a job has 0 iterations. n_events counts ALL events, including those past max_events.
 *
 * HELPERS, host only, pure. iba_sim3_correspondences is the constructor's walk (:62-103) over an iba_fuse_map: the keypoints i1 of keyframe kf1 in
 * ascending order; matches12[i1] < 0, holder(kf1, i1) < 0, either point bad, or either point held by no keypoint of its keyframe: skipped.
 * WHERE A POINT IS HELD TWICE IN A KEYFRAME THE LOWEST KEYPOINT INDEX IS ITS GetIndexInKeyFrame. The thresholds are Z1's from the octave of that
 * keypoint. iba_sim3_sets is the reference's swap-with-back draw (:163-177) over splitmix64. iba_sim3_budget is Z6. iba_sim3_iterate is ONE
 * iterate(n) call as a fold over a finished result: from iteration from_it it walks at most n iterations; the first event among them ends it
 * (*event = its number, *next_it = the iteration after it, *no_more = 0); else *event = -1 and *no_more = (*next_it >= iterations). A TOO_FEW job
 * answers *event = -1, *no_more = 1. iba_sim3_compose is gScm * gSmw of LoopClosing.cc:333-335 in float64: R = Rcm Rmw, t = s (Rcm tmw) + tcm, s.
 * UNPINNED, together: OpenCV's gemm, reduce, dot, cv::eigen and Rodrigues are not vendored and nothing here is compared with recorded OpenCV output;
 * the eigenvector's sign (the rotation does not depend on it); the sets (the reference draws from DUtils::Random; sets is an INPUT so a caller can
 * hand in the reference's own); libm in Z6. KNOWN DEVIATIONS: (1) Z4: the reference goes quaternion -> atan2 -> angle-axis -> cv::Rodrigues; the
 * library forms the same rotation from the quaternion, which keeps libm transcendentals off the device and lets every byte be compared with numpy
 * (profiles/sim3_parity.md measures the difference). (2) Z6's non-finite quotient.
 * NOT PROVIDED: SearchByBoW (it needs the vocabulary), SearchBySim3, OptimizeSim3, the covisibility consistency check, CorrectLoop.
 * DEVICE (csrc/iba_sim3_kernels.hpp), one launch chain per chunk of jobs: preparation (one lane per correspondence, Z2); hypotheses (one lane per
 * (job, iteration), the Jacobi in registers; s, R, t and the two 3 x 4 transforms); the count kernel (Z5, the hot one: J x iterations x N two-way
 * reprojections) in two forms - (a) a lane per hypothesis with the transforms in registers, the correspondences tiled through LDS
 * (IBA_SIM3_TILE per tile) and read at a wave-uniform address, the count in a register; (b) a lane per correspondence, the hypothesis wave-uniform,
 * coalesced loads, the count the popcount of a ballot; profiles/sim3_bench.md records both and names the shipped one -; selection (one wave per
 * job: the best before an iteration is the running maximum of the counts before it, so every lane walks a run of consecutive iterations from a
 * maximum scan's value as Z7 does, and a sum scan numbers the events); flags (the inlier bytes of the listed events and of the best only; per-iteration flags reach global memory
 * only with keep_stages). Counts are integers and nothing is combined by an atomic: no result depends on an arrival order.
 * MEMORY: a call is cut into chunks of consecutive jobs that stay under IBA_SIM3_BUDGET_BYTES, or under a quarter of the device memory free at the
 * call where that is less; a chunk holds at least one job and a chunk boundary changes no byte. The result is host memory.
 * ERRORS, all IBA_ERR_INVALID_ARG with a message (iba_sim3_last_error, per thread) BEFORE the device is touched: a NULL argument (a job's arrays
 * may be NULL only where n == 0; sets only where n < min_inliers) or a wrong struct_size; J < 1; n < 0; a point index outside the table; a pose
 * entry, table point, intrinsic or threshold that is not finite; fx or fy <= 0; probability outside (0, 1); min_inliers < 3; max_iterations outside
 * 1..IBA_SIM3_MAX_ITERATIONS; max_events outside 1..IBA_SIM3_MAX_EVENTS; a set index outside [0, n) or repeated in its set; a job index outside
 * the result; an event index at or above max_events ("raise max_events") or at or above the listed events; a stage accessor on a result without
 * keep_stages. A job with N < min_inliers is legal and gets a status.
 */
#define IBA_SIM3_MAX_ITERATIONS 4096
#define IBA_SIM3_MAX_EVENTS 16
#define IBA_SIM3_TILE 256
#define IBA_SIM3_BUDGET_BYTES (1ull << 30)
typedef enum iba_sim3_status { IBA_SIM3_OK = 0, IBA_SIM3_NO_MORE = 1, IBA_SIM3_TOO_FEW = 2 } iba_sim3_status;
typedef struct iba_sim3_job {                 /* host pointers, read during the call only */
    const float*   Tcw12_1;        /* 3 x 4 row-major float32: keyframe 1's pose */
    const float*   Tcw12_2;        /* keyframe 2's */
    const int32_t* point1;         /* n table indices: mvpMapPoints1 */
    const int32_t* point2;         /* n table indices: mvpMapPoints2 */
    const float*   max_err1;       /* n: Z1 */
    const float*   max_err2;       /* n */
    const int32_t* sets;           /* max_iterations x 3 indices into the correspondence list, distinct inside a set; NULL only where n < min_inliers */
    int32_t n;
    int32_t reserved;              /* 0 */
    float fx1, fy1, cx1, cy1;      /* mK1 */
    float fx2, fy2, cx2, cy2;      /* mK2 */
} iba_sim3_job;
typedef struct iba_sim3_options {
    int32_t struct_size;        /* sizeof(iba_sim3_options) */
    int32_t min_inliers;        /* 20, >= 3 */
    double  probability;        /* 0.99, inside (0, 1) */
    int32_t max_iterations;     /* 300, 1..IBA_SIM3_MAX_ITERATIONS */
    int32_t fix_scale;          /* 0; 1: s = 1.0f */
    int32_t max_events;         /* 1, 1..IBA_SIM3_MAX_EVENTS */
    int32_t keep_stages;        /* 0; 1 keeps every iteration's inlier bytes for iba_sim3_iterations */
} iba_sim3_options;
typedef struct iba_sim3_result {
    int32_t status;             /* iba_sim3_status */
    int32_t n;                  /* N */
    int32_t iterations;         /* Z6; 0 for TOO_FEW */
    int32_t n_events;           /* all of them */
    int32_t n_listed;           /* min(n_events, max_events) */
    int32_t best_it;            /* the iteration of the best after the last one; -1 for TOO_FEW */
    int32_t best_inliers;
    int32_t sweep_cap_hits;     /* iterations whose Jacobi ran to the cap */
} iba_sim3_result;
typedef struct iba_sim3_batch iba_sim3_batch;
iba_status iba_default_sim3_options(iba_sim3_options* opt);
const char* iba_sim3_last_error(void);                               /* never NULL; of this thread's last iba_sim3* call that failed */
/* *out is NULL on failure; release it with iba_sim3_free */
iba_status iba_sim3_solve(const iba_map_points* points, const iba_sim3_job* jobs, int32_t J, const iba_sim3_options* opt, int device, iba_sim3_batch** out);
void       iba_sim3_free(iba_sim3_batch* r);
int32_t    iba_sim3_n_jobs(const iba_sim3_batch* r);                 /* 0 for NULL */
iba_status iba_sim3_read(const iba_sim3_batch* r, int32_t job, iba_sim3_result* result);
/* the inliers of every iteration (`iterations` entries); always available */
iba_status iba_sim3_counts(const iba_sim3_batch* r, int32_t job, int32_t* n_inliers_per_iteration);
/* the k-th event, k < n_listed: its iteration, n_inliers, s, R, t and N inlier bytes; every output may be NULL */
iba_status iba_sim3_event(const iba_sim3_batch* r, int32_t job, int32_t k, int32_t* iteration, int32_t* n_inliers, float* s, float R[9], float t[3], uint8_t* inlier);
/* the same for the best after the last iteration (GetEstimated*); zeros and iteration -1 for a TOO_FEW job */
iba_status iba_sim3_best(const iba_sim3_batch* r, int32_t job, int32_t* iteration, int32_t* n_inliers, float* s, float R[9], float t[3], uint8_t* inlier);
/* keep_stages only: per iteration s (iterations), R (x 9), t (x 3) and the inlier bytes (iterations x N); every output may be NULL */
iba_status iba_sim3_iterations(const iba_sim3_batch* r, int32_t job, float* s, float* R, float* t, uint8_t* inlier);
/* host only, pure: the walk over keyframe kf1's n1 = kp_off[kf1 + 1] - kp_off[kf1] keypoints; matches12[n1] table indices or < 0; the octaves per keypoint
 * of either keyframe, the level tables with n_levels entries; every output takes up to n1 entries (index1: mvnIndices1) and may be NULL; *n their number */
iba_status iba_sim3_correspondences(const iba_fuse_map* map, int32_t kf1, int32_t kf2, const int32_t* matches12, const int32_t* octave1, const int32_t* octave2,
                                    const float* level_sigma2_1, const float* level_sigma2_2, int32_t n_levels1, int32_t n_levels2, int32_t* index1, int32_t* point1,
                                    int32_t* point2, float* max_err1, float* max_err2, int32_t* n);
/* host only, pure: iterations x 3 indices, distinct inside a set; N >= 3 */
iba_status iba_sim3_sets(int32_t N, int32_t iterations, uint64_t seed, int32_t* out);
/* host only, pure: Z6; N >= 1 */
iba_status iba_sim3_budget(int32_t N, const iba_sim3_options* opt, int32_t* iterations);
/* host only, pure: one iterate(n) of the reference over a finished result; 0 <= from_it <= iterations, n >= 0 */
iba_status iba_sim3_iterate(const iba_sim3_batch* r, int32_t job, int32_t from_it, int32_t n, int32_t* next_it, int32_t* event, int32_t* no_more);
/* host only, pure: Scw = Scm * Smw in float64; Tmw12 is the matched keyframe's pose (3 x 4 float32) */
iba_status iba_sim3_compose(float s, const float R[9], const float t[3], const float* Tmw12, double* s_out, double R_out[9], double t_out[3]);

/*
 * ---- Bundle adjustment [the camera side's fifth brick: the reference's Optimizer::BundleAdjustment (src/orb_slam/src/Optimizer.cc:215-407: the global
 * BA of Tracking::CreateInitialMapMonocular, Tracking.cc:686, and of LoopClosing.cc:651) and Optimizer::LocalBundleAdjustment from its "Setup
 * optimizer" on (:671-937, LocalMapping.cc:80)] ----
 * A call takes B independent jobs on one device. A job is n_cameras poses Tcw (3 x 4 row-major, float64) with a `fixed` byte each, n_points points
 * (float32, widened as Converter::toVector3d does), n_edges monocular edges (point, camera, undistorted keypoint position, the information of the
 * keypoint's pyramid level) IN ANY ORDER, and one set of pinhole intrinsics. Camera poses AND points are optimised together by Levenberg-Marquardt on
 * the point-marginalised (Schur) reduced camera system. STEREO EDGES ARE NOT PROVIDED (as in iba_pose), pbStopFlag IS NOT PROVIDED, and a job has at
 * most IBA_BUNDLE_MAX_FREE_CAMERAS cameras that are not fixed (a reduced system of 384 unknowns): a global BA over a larger map is out of scope.
 * ARITHMETIC. float64, every operation rounded, left to right as written, no contraction, nothing but + - x / sqrt up to a step of theta = pi (P6).
 * A NaN stored into an output is the canonical quiet NaN. The device and the host restatement (iba_debug_bundle_host, the same text of arithmetic:
 * csrc/iba_bundle_math.hpp) agree byte for byte; the order of every sum is a function of the job's own index arrays alone and never of the batch, the
 * chunk, the grid or the launch shape.
 *
 *   B1 edge.       p = R X + t, the error e, chi2 and the 2 x 6 pose Jacobian Jc are exactly P1's (pose::edge, not written again). The 2 x 3 point
 *                  Jacobian is that of EdgeSE3ProjectXYZ::linearizeOplus, -(1/p_z) [fx, 0, -fx p_x/p_z; 0, fy, -fy p_y/p_z] R, associated as: iz =
 *                  1 / p_z, a = (-(fx p_x)) iz, b = (-(fy p_y)) iz; Jl_0c = (-iz) (fx R_0c + a R_2c), Jl_1c = (-iz) (fy R_1c + b R_2c) (the literal
 *                  zeros are left out). isDepthPositive is p_z > 0 at the current estimates (false for a NaN).
 *   B2 Huber.      P2. w = rho' inv_sigma2 scales all of Hpp, Hll, Hpl, bp, bl: Hpp_pq += w (Jc_0p Jc_0q + Jc_1p Jc_1q) (p <= q), bp_p -= w (Jc_0p e_x
 *                  + Jc_1p e_y), Hll and bl likewise from Jl, and W = Hpl (6 x 3) of ONE edge is W_rc = w (Jc_0r Jl_0c + Jc_1r Jl_1c).
 *   B3 sums.       A free camera's 21 + 6 sums run over its edges in ascending edge index: the k-th edge of that list (active or not) belongs to
 *                  lane k mod 64, a lane adds its ACTIVE edges in ascending k onto +0.0, and the 64 lane sums are combined by the balanced tree
 *                  v[l] = v[2l] + v[2l + 1] (one wave per camera, the DPP sum of iba_pose). A point's 6 + 3 sums and its robust chi2 partial are
 *                  sequential over its active edges in ascending edge index (one lane per point). The job's robust chi2 is the sum of the partials
 *                  of the participating points under P3's rule with point p on lane p mod 256.
 *   B4 what takes part. A point with no active edge is left out and keeps its value (g2o's initializeOptimization(level)). A free camera with no
 *                  active edge is left out likewise: its step is zero and it has NO ROW in the reduced system, whose rows are the participating
 *                  free cameras in ascending camera index. A fixed camera contributes to Hll and bl only.
 *   B5 point blocks. Per participating point A = Hll + lambda I is inverted by cofactors: c00 = a11 a22 - a12 a12, c01 = a02 a12 - a01 a22, c02 = a01
 *                  a12 - a02 a11, c11 = a00 a22 - a02 a02, c12 = a01 a02 - a00 a12, c22 = a00 a11 - a01 a01, det = (a00 c00 + a01 c01) + a02 c02,
 *                  A^-1_ij = c_ij (1 / det). A det that is not positive and finite fails the trial as P4's pivot does.
 *   B6 Schur.      S_ab = [a == b](Hpp_a + lambda I) - sum_p W_pa A_p^-1 W_pb^T and bs_a = bp_a - sum_p W_pa A_p^-1 bl_p. The blocks (a <= b, both
 *                  free) and per block its items (point, edge of a, edge of b), points ascending, are a host-side plan of the indices alone
 *                  (iba_bundle_plan); outliers only mask items. Per item Y = W_a A^-1 with Y_rc = (W_r0 A_0c + W_r1 A_1c) + W_r2 A_2c, the term
 *                  G_rs = (Y_r0 Wb_s0 + Y_r1 Wb_s1) + Y_r2 Wb_s2 and, in a diagonal block, g_r = (Y_r0 bl_0 + Y_r1 bl_1) + Y_r2 bl_2. A block's 36
 *                  (+ 6) sums follow the camera rule: the k-th item of its list on lane k mod 64, active items ascending onto +0.0, the tree. Only
 *                  the lower triangle of S is formed: entry (6 rb + s, 6 ra + r) = -G_rs for a < b, and (6 ra + r, 6 ra + s), s <= r, = (Hpp_sr +
 *                  [r == s] lambda) - G_rs on the diagonal.
 *   B7 solve.      Cholesky without pivoting, entry by entry: d = s_jj - sum_{k<j} l_jk l_jk, l_jj = sqrt(d), l_ij = (s_ij - sum_{k<j} l_ik l_jk) /
 *                  l_jj, k ascending, each product subtracted from the running value one at a time. y_i = (bs_i - sum_{k<i} l_ik y_k) / l_ii, k
 *                  ascending; dp_i = (y_i - sum_{k>i} l_ki dp_k) / l_ii, k DESCENDING from the last row. A d that is not positive and finite is a
 *                  failed trial. The kernel runs the columns in parallel (one lane per row) and gives the same bytes. Then per participating point
 *                  dl = A^-1 (bl - sum_a W_pa^T dp_a): v_c = bl_c, and per active edge of the point with a camera that has a row, ascending, v_c
 *                  -= (((((W_0c d0 + W_1c d1) + W_2c d2) + W_3c d3) + W_4c d4) + W_5c d5); dl_c = (A_c0 v0 + A_c1 v1) + A_c2 v2. Cameras are
 *                  updated by P6 (unchanged), points by X + dl.
 *   B8 LM.         P5, generalised in three places: lambda at iteration 0 of every round is 1e-5 x the largest |diagonal| over the Hpp AND the
 *                  Hll of the participating vertices; scale = 1e-3 + sum dx (lambda dx + b) over every participating unknown, one running sum,
 *                  cameras ascending then points ascending; the trial's chi2 is B3's. The 10-trial rule, the acceptance, the alpha clamp, ni and
 *                  the stops are P5's. A failed B5 or B7 is P4's failed trial.
 *   B9 schedule.   A round continues from the previous round's estimate (LocalBundleAdjustment never resets it). After round r < rounds - 1
 *                  every still-active edge with (float)chi2 > chi2_threshold or without positive depth is deactivated for good (setLevel(1) is
 *                  never undone). The kernel is on for rounds < robust_rounds. After the last round every edge, active or not, is classified at
 *                  the final estimates into the reported outlier flag and float32 chi2: the reference's vToErase is the flagged (camera, point)
 *                  pairs. Per round: chi2 (the robust sum over the round's active edges at its final estimate), n_bad (edges deactivated so far;
 *                  for the last round the flagged edges), lm_iterations (begun), trials. n_edges == 0 is legal and changes nothing.
 *   B10 plan.      Edges come in any order; the per-point and per-camera lists are stable in edge index. A (point, camera) pair that occurs twice
 *                  is refused: the reference's std::map<KeyFrame*, size_t> cannot hold one.
 *
 * UNPINNED, together (g2o is third party and absent): the associations of B1 and B2, all of B5-B7 (g2o's block solver and Eigen's or CSparse's
 * factorisation), B8 and the order of every sum. KNOWN DEVIATIONS: the two of iba_pose: the given poses are never re-orthonormalised, and classification is
 * at the accepted estimate; g2o's chi2() of an edge at level 1 is stale from the first round, here every edge is evaluated at the final estimates;
 * the edge order inside a point is ascending edge index where the reference's is pointer order.
 * DEVICE (csrc/iba_bundle_kernels.hpp): ONE LAUNCH CHAIN PER LM EVALUATION over the flat tables of all jobs of a chunk - edges (one lane each), point
 * and camera sums, the job's chi2 and the sequencer's first half (one workgroup per job, one lane sequencing), point inverses, the blocks of the
 * reduced system (one wave each), the factorisation (one workgroup per job, the matrix in global memory), the steps and trial estimates, the
 * sequencer's second half - so one large job and a thousand small ones both fill the machine. No workgroup waits for another: kernel boundaries are
 * the only grid-wide synchronisation. The host reads ONE word per step (the jobs still running) and stops enqueuing at zero; it does no arithmetic
 * between the upload and the download. Chunks of consecutive jobs run under 1 GiB, or a quarter of the free device memory where that is less; a job
 * above the budget is a chunk of its own; a chunk boundary changes no byte.
 * ERRORS, all IBA_ERR_INVALID_ARG with a message (iba_bundle_last_error, per thread) BEFORE the device is touched: a NULL argument (a job's arrays
 * may be NULL only where their count is 0) or a wrong struct_size; B < 1; a count outside 0..IBA_BUNDLE_MAX_COUNT; a pose, point, observation,
 * information or intrinsic that is not finite; fx or fy <= 0; inv_sigma2 < 0; an edge's point or camera out of range; a duplicate (point, camera);
 * more than IBA_BUNDLE_MAX_FREE_CAMERAS free cameras; 2^31 pair items or more; rounds outside 1..4, iterations[r] outside 1..100, robust_rounds
 * outside 0..4, a threshold or delta that is not finite, chi2_threshold < 0, huber_delta <= 0; a job or round index outside the result; the stage
 * accessor on a result without keep_stages.
 * AFTER A CALL the reference runs UpdateNormalAndDepth() on every point it moved (Optimizer.cc:397, :936, :1200): write the optimised poses and
 * points into the keyframe and point tables and call iba_refresh (S4 / S5 of the map-point refresh, above) on the moved points.
 */
#define IBA_BUNDLE_MAX_FREE_CAMERAS 64
#define IBA_BUNDLE_MAX_ROUNDS 4
#define IBA_BUNDLE_MAX_COUNT (1 << 24)        /* of a job's cameras, points and edges each: every index fits int32 */
typedef struct iba_bundle_job {               /* host pointers, read during the call only */
    const double*  Tcw12;        /* n_cameras x 12 */
    const uint8_t* fixed;        /* n_cameras: 1 = the camera is not optimised (keyframe 0, the fixed cameras of a local window) */
    const float*   xyz;          /* n_points x 3: MapPoint::GetWorldPos */
    const int32_t* edge_point;   /* n_edges */
    const int32_t* edge_camera;  /* n_edges */
    const float*   obs;          /* n_edges x 2: mvKeysUn[i].pt */
    const float*   inv_sigma2;   /* n_edges: mvInvLevelSigma2[octave] */
    int32_t n_cameras, n_points, n_edges;
    float fx, fy, cx, cy;
} iba_bundle_job;
typedef struct iba_bundle_options {
    int32_t struct_size;                          /* sizeof(iba_bundle_options) */
    int32_t rounds;                               /* 2, 1..4 */
    int32_t iterations[IBA_BUNDLE_MAX_ROUNDS];    /* {5, 10}, 1..100 each */
    int32_t robust_rounds;                        /* 1: the Huber kernel is off after this many rounds */
    float   chi2_threshold;                       /* 5.991f */
    float   huber_delta;                          /* (float)sqrt(5.991); the global schedule: (float)sqrt(5.99), as BundleAdjustment writes it */
    int32_t keep_stages;                          /* 0; 1 allows iba_bundle_stage */
} iba_bundle_options;
typedef struct iba_bundle_result {
    int32_t n_cameras, n_points, n_edges, n_free;
    int32_t n_outliers;                           /* the edges flagged by the last classification */
    int32_t rounds_run;
    double  chi2[IBA_BUNDLE_MAX_ROUNDS];
    int32_t n_bad[IBA_BUNDLE_MAX_ROUNDS], lm_iterations[IBA_BUNDLE_MAX_ROUNDS], trials[IBA_BUNDLE_MAX_ROUNDS];
} iba_bundle_result;
/* what iba_bundle_eval fills per job: every pointer may be NULL (not wanted). A camera or point that does not take part (B4) reports zeros. */
typedef struct iba_bundle_eval_out {
    double* Hpp;          /* n_cameras x 36, both triangles */
    double* bp;           /* n_cameras x 6 */
    double* Hll;          /* n_points x 9 */
    double* bl;           /* n_points x 3 */
    double* chi2_edges;   /* n_edges: every edge's chi2 (no kernel), active or not */
    double* S;            /* n_reduced x n_reduced, both triangles mirrored from the lower one; room for (6 x free cameras)^2 */
    double* bs;           /* n_cameras x 6 */
    double* dp;           /* n_cameras x 6 */
    double* dl;           /* n_points x 3 */
    double  chi2_robust, lambda;
    int32_t n_reduced;    /* 6 x the participating free cameras */
    int32_t solved;       /* 0: B5 or B7 failed; S, bs, dp, dl are zeros */
} iba_bundle_eval_out;
typedef struct iba_bundle_batch iba_bundle_batch;
iba_status iba_default_bundle_options(iba_bundle_options* opt);     /* the local schedule: 2 rounds of {5, 10}, the first robust */
/* the global schedule: one round of n_iterations (1..100), the Huber kernel on where robust != 0, delta = (float)sqrt(5.99) */
iba_status iba_bundle_options_global(iba_bundle_options* opt, int32_t n_iterations, int32_t robust);
const char* iba_bundle_last_error(void);                            /* never NULL; of this thread's last iba_bundle* call that failed */
/* *out is NULL on failure; release it with iba_bundle_free */
iba_status iba_bundle_optimize(const iba_bundle_job* jobs, int32_t B, const iba_bundle_options* opt, int device, iba_bundle_batch** out);
/* one linearisation per job AT the job's estimates and one step at the given lambda (B1-B7, delta = (float)sqrt(5.991)): active is NULL (all edges of
 * all jobs) or one pointer per job (NULL = all, else n_edges bytes); outs takes B entries whose pointers the caller has set */
iba_status iba_bundle_eval(const iba_bundle_job* jobs, int32_t B, const uint8_t* const* active, int32_t robust, double lambda, int device, iba_bundle_eval_out* outs);
void       iba_bundle_free(iba_bundle_batch* r);
int32_t    iba_bundle_n_jobs(const iba_bundle_batch* r);            /* 0 for NULL */
iba_status iba_bundle_read(const iba_bundle_batch* r, int32_t job, iba_bundle_result* result);
/* the final poses: n_cameras x 12 each; either may be NULL. Tcw12f is the rounding of Converter::toCvMat */
iba_status iba_bundle_cameras(const iba_bundle_batch* r, int32_t job, double* Tcw12, float* Tcw12f);
iba_status iba_bundle_points(const iba_bundle_batch* r, int32_t job, double* xyz, float* xyzf);   /* n_points x 3 each; either may be NULL */
/* per edge the outlier flag and the float32 chi2 of the last classification (n_edges each); either may be NULL */
iba_status iba_bundle_edges(const iba_bundle_batch* r, int32_t job, uint8_t* outlier, float* chi2);
/* keep_stages only: the estimates at the end of round `round` < rounds_run; either may be NULL */
iba_status iba_bundle_stage(const iba_bundle_batch* r, int32_t job, int32_t round, double* Tcw12, double* xyz);
/* host only, pure (B6, B10): the plan of one job. point_offsets (n_points + 1), point_edges (n_edges), camera_offsets (n_cameras + 1), camera_edges
 * (n_edges), block_cameras (2 per block), block_offsets (n_blocks + 1) and items (point, edge of a, edge of b: 3 per item) may each be NULL; n_blocks
 * and n_items are always written, so a first call sizes the arrays of a second */
iba_status iba_bundle_plan(const iba_bundle_job* job, int32_t* point_offsets, int32_t* point_edges, int32_t* camera_offsets, int32_t* camera_edges, int32_t* n_blocks,
                           int32_t* n_items, int32_t* block_cameras, int32_t* block_offsets, int32_t* items);
/* host only, pure: the joining helper of one LocalMapping step, Optimizer.cc:620-669 and the vertex and edge order of :682-779 over the map's
 * observation table. observations: n_observations rows (map point, keyframe, keypoint), ids counting from 0; point_bad (n_map_points) and
 * keyframe_bad (n_keyframes) are the isBad() flags; covisible: the current keyframe's GetVectorCovisibleKeyFrames in the caller's order. Out:
 *   camera_keyframe, fixed (up to n_keyframes)  the job's cameras as keyframe ids: the *n_local local ones (the current one first, then the covisibles
 *                                that are not bad), then the fixed ones in first-seen order; fixed = 1 for keyframe 0 and for every fixed camera
 *   point_id (up to n_map_points) the local points in the reference's walk order: per local camera its map points in ascending keypoint index, a
 *                                point that is not bad and not yet listed
 *   edge_point, edge_camera, edge_keypoint (up to n_observations)  per local point its observations by keyframes that are not bad, in ASCENDING
 *                                KEYFRAME ID (the reference's order is that of the keyframes' addresses): the job's index arrays, and the keypoint
 *                                whose mvKeysUn position and octave give obs and inv_sigma2
 * Refused: an id out of range, a (map point, keyframe) or (keyframe, keypoint) pair that occurs twice, a covisible that is the current keyframe or
 * is listed twice, a NULL array that would be written. */
iba_status iba_bundle_local_window(const int32_t* observations, int32_t n_observations, const uint8_t* point_bad, int32_t n_map_points, const uint8_t* keyframe_bad,
                                   int32_t n_keyframes, int32_t current, const int32_t* covisible, int32_t n_covisible, int32_t* camera_keyframe, uint8_t* fixed,
                                   int32_t* n_local, int32_t* n_cameras, int32_t* point_id, int32_t* n_points, int32_t* edge_point, int32_t* edge_camera,
                                   int32_t* edge_keypoint, int32_t* n_edges);

/* The ABI version the LIBRARY was built with (IBA_ABI_VERSION of its header). iba_params carries no struct_size: a caller compiled against
 * an older header would pass a shorter struct. Callers compare iba_abi_version() with their own IBA_ABI_VERSION before iba_create(). */
int32_t iba_abi_version(void);
/* The HIP device a handle lives on (the `device` it was created with; a handle of iba_submap_handle: its source's); -1 for NULL. */
int32_t iba_handle_device(const iba_handle* h);

/* Output of one BAError() call. The first five fields are the reference's returned tuple
 * (iba_global.cpp:343); the rest are the counters it prints with verborse (:341-342). */
typedef struct iba_cost_out {
    double f1;               /* mean 3d-2d distance over valid edges, DBL_MAX sentinel (:330-333) */
    double f2;               /* mean 3d-3d distance over valid edges, DBL_MAX sentinel (:334-337) */
    double C;                /* mean hand-eye constraint value, NaN if no frame was processed (:338) */
    int32_t valid_cnt_3d_2d;
    int32_t cnt_3d_2d;
    int32_t cnt_3d_3d;
    int32_t valid_cnt_3d_3d;
    int32_t valid_pl_3d_3d;
    int32_t valid_pt_3d_3d;
    int32_t frames_used;     /* frames that passed the >= num_min_corr_cost test */
    int32_t n_corr;          /* sum of corrset.size() over used frames */
} iba_cost_out;

/* Gauss-Newton normal equations of the iba_local problem at x:
 *   H = sum_blocks w J^T J,  b = sum_blocks w J^T r,  cost = 1/2 sum_blocks rho(|r|^2)
 * with Huber IRLS weights per residual block as Ceres applies them (corrector with rho''<=0). */
typedef struct iba_normal_out {
    double H[49]; /* row-major symmetric 7x7 */
    double b[7];
    double cost;          /* Ceres convention: 1/2 sum rho(s) */
    double chi2;          /* sum |r|^2 (un-robustified) */
    int32_t n_factor_3d2d; /* IBA_PlaneFactor blocks (factor_3d2d_kind = 1: IBATestEdge blocks) */
    int32_t n_factor_p2pl; /* Point2Plane_Factor blocks */
    int32_t n_factor_p2pt; /* Point2Point_Factor blocks */
    int32_t n_residuals;   /* total scalar residuals */
    int32_t frames_used;
    int32_t n_corr;
} iba_normal_out;

/* NOMAD black-box outputs of BALoss::eval_x (iba_global.cpp:386-392). */
typedef struct iba_bbo {
    double f, c1, c2, c3;
} iba_bbo;

iba_status iba_default_params(iba_params* p); /* IBAGlobalParams / IBALocalParams defaults */

/* Uploads the frames [frame_begin, frame_end) of the problem to HIP device `device`, builds the
 * static per-scan 3-D indices (reference: KDTree3D per scan, iba_global.cpp:361-367) and the
 * per-frame keypoint grids. The full descriptor must be given on every rank (covisible keypoints
 * are resolved at creation time); only owned frames are uploaded and evaluated. */
iba_status iba_create(const iba_problem_desc* desc, const iba_params* params, int device,
                      int32_t frame_begin, int32_t frame_end, iba_handle** out);
/*
 * Engine options of a handle (no reference counterpart: none of them changes a result bit, they steer how the work is shared
 * between candidates and calls). Fill with iba_default_create_options, change fields, pass to iba_create_ex; iba_create uses the
 * defaults. The IBA_* environment variables of earlier rounds are still read at creation as DEBUG overrides of these fields
 * (process-global, for A/B runs without recompiling a caller); an integrator sets the struct.
 */
typedef struct iba_create_options {
    int32_t struct_size;          /* sizeof(iba_create_options) of the caller: the struct may grow at its end */
    int32_t common_pairs;         /* 2d-3d pair search shared by a batch: 0 never, 1 when the batch (or each of its groups) is tight [default], 2 always */
    double common_max_px;         /* nominal projection spread (px) up to which candidates share one pair search [20] */
    int32_t max_pair_groups;      /* a wider batch is clustered into up to this many tight groups, 1..4 [4]; 1 = no clustering */
    int32_t pair_memo;            /* pair lists built for an inflated bound and reused by later calls that stay inside it [1] */
    int32_t pair_memo_max_batch;  /* largest batch (group) whose lists are built reusable [40] */
    double pair_inflation;        /* inflation of a reusable list's bound [1.25] */
    int32_t anchored_lists;       /* 3-D 1-NN memoised around an anchor extrinsic that follows the candidates [1] */
    double anchor_reach;          /* drift (m) of a MapPoint query 30 m out that moves the anchor [0.06] */
    int32_t side_stream;          /* (round 3-4: staging launch on a second stream of the handle) no effect since round 5: the chain has no staging launch [1] */
    int32_t spin_wait;            /* the host polls the stream at the end of a call instead of blocking [1] */
    int32_t factor_mfma;          /* normal-equation sums on the matrix cores (v_mfma_f64_16x16x4; measured slower) [0] */
    int32_t pair_list_capacity;   /* entries per keyframe of a pair list; 0 = automatic. A full list only costs speed [0] */
    int32_t max_chain_batch;      /* candidates one launch chain takes, 1..IBA_MAX_CHAIN [512]: a shard of few keyframes (one rank of an 8-GPU job) fills the
                                     device only with many candidates per chain. Work lists are allocated for the largest batch a call has passed so far
                                     (16 B x keypoints x keyframes per candidate); with plane_cache = 0 a chain takes at most IBA_MAX_BATCH */
    int32_t chain_fold;           /* 1: the candidate block reaches the device through spare blocks of the first kernel of the chain and the hand-eye terms
                                     are evaluated inside the summing kernel (no staging launch, no second stream, no event between kernels) [1];
                                     0: a staging launch of its own at the head of every chain */
} iba_create_options;
iba_status iba_default_create_options(iba_create_options* o);
iba_status iba_create_ex(const iba_problem_desc* desc, const iba_params* params, int device,
                         int32_t frame_begin, int32_t frame_end, const iba_create_options* options, iba_handle** out);
void iba_destroy(iba_handle* h);
iba_status iba_set_params(iba_handle* h, const iba_params* params);
const char* iba_last_error(const iba_handle* h); /* never NULL; h may be NULL for creation errors */

/* BAError() for B candidate x = [omega(3), upsilon(3), s] (row-major B x 7). */
iba_status iba_eval_cost(iba_handle* h, const double* x, int32_t B, iba_cost_out* out);
/* BALoss::eval_x packing on top of iba_eval_cost. */
iba_status iba_eval_bbo(iba_handle* h, const double* x, int32_t B, double he_threshold, double valid_rate,
                        iba_bbo* out);

/* BuildProblem() at x_assoc followed by one evaluation of every residual block at the same x:
 * association + residuals + Jacobians + normal equations, B candidates per call. */
iba_status iba_eval_normal(iba_handle* h, const double* x, int32_t B, iba_normal_out* out);

/* BAError tuple AND the re-associated normal equations of the same B candidates from one pass over the scans
 * (the two paths share projection + 2d-3d association). Counters are identical to those of iba_eval_cost and
 * iba_eval_normal called separately, sums agree to summation order (1e-15). A candidate's results do not depend on what
 * else is in the batch. */
iba_status iba_eval_full(iba_handle* h, const double* x, int32_t B, iba_cost_out* cost, iba_normal_out* normal);

/* The two halves separately, as Ceres uses them (iba_local.cpp:443-445): freeze the association
 * at x_assoc, then evaluate the frozen residual blocks at B other x. */
iba_status iba_build_problem(iba_handle* h, const double* x_assoc);
iba_status iba_eval_factors(iba_handle* h, const double* x, int32_t B, iba_normal_out* out);
/* The frozen problem as ONE residual block for a solver that wants residuals and Jacobians (Ceres: the blocks
 * BuildProblem() adds, iba_local.cpp:263-308; g2o: a unary edge on VertexSim3, IBACalib.hpp:74-155): 8 rows with
 *   J^T J = H,  J^T r = b,  |r|^2 = 2 cost      ([J | r] = upper Cholesky factor of [[H, b], [b^T, 2 cost]])
 * so that the solver's Gauss-Newton model AND its step-acceptance cost are those of the whole problem, robust weights
 * included. r has 8 entries, J is 8 x 7 row-major. iba_whiten_normal is the host-only half (any iba_normal_out). */
iba_status iba_eval_whitened(iba_handle* h, const double* x, double r[8], double J[56]);
iba_status iba_whiten_normal(const iba_normal_out* normal, double r[8], double J[56]);
/* Caller of the Jacobian path: the outer re-association loop of iba_local
 * (iba_local.cpp:434-460) around a Ceres-style LM on the device-reduced 7x7 normal equations. */
typedef struct iba_lm_options {
    int32_t max_outer_iterations; /* max_iba_iter */
    int32_t max_inner_iterations; /* 30, iba_local.cpp:437 */
    double min_diff;              /* iba_min_diff for allClose (iba_local.cpp:454) */
    double function_tolerance, gradient_tolerance, parameter_tolerance; /* Ceres defaults 1e-6, 1e-10, 1e-8 */
    double initial_trust_region_radius;                                 /* 1e4 */
} iba_lm_options;
typedef struct iba_lm_result {
    double x[7];
    int32_t outer_iterations, inner_iterations, evaluations, converged;
    double initial_cost, final_cost;
} iba_lm_result;
iba_status iba_default_lm_options(iba_lm_options* o);
iba_status iba_calibrate_lm(iba_handle* h, const double* x0, const iba_lm_options* opt, iba_lm_result* res);

/* Per-residual values and Jacobians of the frozen problem (for Ceres / g2o adaptors and tests).
 * Call with r == NULL to query *n_rows. J is n_rows x 7 row-major, block_id[n_rows] identifies the
 * residual block, block_kind: 0 = IBA_PlaneFactor, 1 = Point2Plane, 2 = Point2Point, 3 = IBATestEdge (factor_3d2d_kind = 1). */
iba_status iba_eval_residuals(iba_handle* h, const double* x, double* r, double* J, int32_t* block_id,
                              int32_t* block_kind, int64_t* n_rows);

/* 2d-3d correspondences (corrset of FindProjectCorrespondences, iba_global.cpp:55-96) of one owned
 * frame at x: pairs (keypoint id, scan point id) sorted by keypoint id. cap = capacity in pairs. */
iba_status iba_get_correspondences(iba_handle* h, const double* x, int32_t frame, uint32_t* kp_idx,
                                   uint32_t* pt_idx, int32_t cap, int32_t* n_out);

/*
 * Multi-GPU building blocks (frames shard across ranks; one sum all-reduce per evaluation).
 * iba_eval_*_partial writes this rank's partial sums for B candidates into DEVICE memory
 * `d_partials` (B * iba_partial_stride() doubles, counters carried as doubles) on HIP stream
 * `stream` (a hipStream_t passed as void*; NULL = the handle's own NON-BLOCKING stream, NOT the legacy default stream: a caller whose
 * other work — the all-reduce, copies — sits on the default stream must pass a stream of its own) without synchronising.
 * After the caller has summed the partial blocks over ranks (ncclAllReduce, sum, f64),
 * iba_finalize_* turns HOST copies of the summed blocks into the outputs above.
 */
int32_t iba_partial_stride(void);
iba_status iba_eval_cost_partial(iba_handle* h, const double* x, int32_t B, void* d_partials, void* stream);
iba_status iba_eval_normal_partial(iba_handle* h, const double* x, int32_t B, void* d_partials, void* stream);
/* cost and normal sums share one block (disjoint slots): finalize the summed block with BOTH iba_finalize_* */
iba_status iba_eval_full_partial(iba_handle* h, const double* x, int32_t B, void* d_partials, void* stream);
iba_status iba_finalize_cost(const iba_params* params, const double* partials, int32_t B, iba_cost_out* out);
iba_status iba_finalize_normal(const iba_params* params, const double* partials, int32_t B, iba_normal_out* out);

/* The frozen problem's residual blocks, as a partial block (the Jacobian-path half of the LM caller on several GPUs). */
iba_status iba_eval_factors_partial(iba_handle* h, const double* x, int32_t B, void* d_partials, void* stream);
/* Calls on one handle must be issued in order, on one stream at a time: the handle's work buffers (candidate ring, lists,
 * records) are reused from call to call and are ordered by that stream only.
 * A cost evaluation also uses a second stream that belongs to the handle: its staging launch (candidates -> device, hand-eye terms)
 * and the later copy of the candidates' derivatives run there, beside the pair search / the search kernel on `stream`. That stream
 * is ordered behind everything `stream` held when the call was made and `stream` waits for it before the first kernel that reads
 * its results, so a caller sees one stream's ordering (IBA_SIDE_STREAM=0 in the environment: everything on `stream`). */

/* Diagnostics, timing probes and self-tests (iba_debug_*, iba_last_*_ms, iba_set_timing, iba_*_selftest*) are declared in
 * iba_mi355x_debug.h: test and benchmark tooling, not part of the drop-in surface. */
int64_t iba_num_points(const iba_handle* h);
int64_t iba_num_keypoints(const iba_handle* h);
int64_t iba_frame_num_points(const iba_handle* h, int32_t frame);   /* points of one local frame; -1 for NULL or a frame out of range */

/*
 * Batch-aware mesh adaptive direct search for the global stage [SURVEY.md 8(f) row 2]: the caller the reference gets
 * from NOMAD 4 (iba_global.cpp:551-602: 7 variables, bounds x0 + lb / x0 + ub, OBJ + 3 progressive-barrier
 * constraints from BALoss::eval_x, OrthoMADS 2N, INITIAL_POLL_SIZE, MIN_MESH_SIZE, MAX_BB_EVAL). One iteration =
 * one iba_eval_bbo batch (full polls around the feasible and the infeasible incumbent). csrc/iba_mads.hpp.
 */
typedef struct iba_mads_options {
    int32_t max_bb_eval;     /* max_bbeval, 5000 */
    double lb[7], ub[7];     /* ABSOLUTE bounds (the reference adds its yml lb/ub to x0, iba_global.cpp:530-533) */
    double init_frame[7];    /* init_frame, 0.5 each */
    double min_mesh;         /* min_mesh, 1e-6 */
    double he_threshold;     /* constraint |C| <= he_threshold (iba_global.cpp:387) */
    double valid_rate;       /* constraint valid/(cnt+1) >= valid_rate (:388) */
    int32_t seed;
    int32_t bases_per_poll;  /* orthogonal 2n-direction sets per poll centre and iteration (1 = OrthoMADS 2N) */
    int32_t speculative;     /* 1: one extra point along the last successful direction */
    int32_t vns_max_idle;    /* variable-neighbourhood restarts (use_vns): stop after this many in a row without gain; 0 = none */
} iba_mads_options;
typedef struct iba_mads_result {
    double x[7];
    double f, c1, c2, c3;
    int32_t feasible;        /* 1: x satisfies the three constraints (findBestFeas, iba_global.cpp:593-599) */
    int32_t evaluations, iterations, batches, cache_hits, restarts;
    int32_t stop_reason;     /* 1 converged (min mesh, restarts exhausted), 2 evaluation budget */
} iba_mads_result;
/* defaults of config/calib/00/iba_calib_global.yml:21-47 around x0 (lb/ub = x0 -/+ (0.1,0.1,0.1,0.3,0.3,0.3,1.0)) */
iba_status iba_default_mads_options(const double* x0, iba_mads_options* o);
iba_status iba_calibrate_mads(iba_handle* h, const double* x0, const iba_mads_options* opt, iba_mads_result* res);
/*
 * Multi-GPU inside one process: the keyframes sharded over n devices of a node (contiguous ranges balanced by points), one
 * handle, one issuing thread and one RCCL communicator per device (ncclCommInitAll). The reference's one parallel strategy is the
 * frame loop with critical-section sums (iba_global.cpp:193, 239, 318; iba_func.cpp:203; iba_local.cpp:162); here every device
 * evaluates its frames, ONE ncclAllReduce(sum, f64) of the B x iba_partial_stride() block over xGMI adds them on the devices,
 * and device 0's copy is finalised on the host. Same outputs and callers as the single-device entry points. The candidate
 * block (Sim3Exp and its derivatives) is computed once per call, the devices are issued concurrently, and the caller's current
 * HIP device is left alone. librccl is loaded (dlopen) when the first communicator is needed: single-device and host-only
 * users of this library do not need it installed.
 */
typedef struct iba_group iba_group;
iba_status iba_group_create(const iba_problem_desc* desc, const iba_params* params, const int32_t* devices, int32_t n_devices, iba_group** out);
/* flags: IBA_GROUP_REDUCE_HOST = the partial blocks are copied to the host and summed there in rank order (bitwise
 * reproducible, no RCCL needed, and the same device may appear more than once in `devices`) instead of one ncclAllReduce */
#define IBA_GROUP_REDUCE_HOST 1
iba_status iba_group_create_ex(const iba_problem_desc* desc, const iba_params* params, const int32_t* devices, int32_t n_devices, int32_t flags, iba_group** out);
void iba_group_destroy(iba_group* g);
const char* iba_group_last_error(const iba_group* g); /* g may be NULL for creation errors */
int32_t iba_group_size(const iba_group* g);
int32_t iba_group_comm_ranks(const iba_group* g);     /* ncclCommCount of the group's communicator; 0 with IBA_GROUP_REDUCE_HOST */
double iba_group_last_issue_us(const iba_group* g);   /* host wall time of the last chunk: candidate block, hand-over to the device threads, wait */
double iba_group_last_enqueue_us(const iba_group* g); /* of which: until the last device's launch chain + collective were enqueued (host issue time) */
iba_status iba_group_frame_range(const iba_group* g, int32_t rank, int32_t* frame_begin, int32_t* frame_end);
iba_status iba_group_set_params(iba_group* g, const iba_params* params);
iba_status iba_group_eval_cost(iba_group* g, const double* x, int32_t B, iba_cost_out* out);
iba_status iba_group_eval_bbo(iba_group* g, const double* x, int32_t B, double he_threshold, double valid_rate, iba_bbo* out);
iba_status iba_group_eval_normal(iba_group* g, const double* x, int32_t B, iba_normal_out* out);
iba_status iba_group_eval_full(iba_group* g, const double* x, int32_t B, iba_cost_out* cost, iba_normal_out* normal);
iba_status iba_group_build_problem(iba_group* g, const double* x_assoc);
iba_status iba_group_eval_factors(iba_group* g, const double* x, int32_t B, iba_normal_out* out);
iba_status iba_group_calibrate_lm(iba_group* g, const double* x0, const iba_lm_options* opt, iba_lm_result* res);
iba_status iba_group_calibrate_mads(iba_group* g, const double* x0, const iba_mads_options* opt, iba_mads_result* res);
/* One process per GPU with a communicator of the caller's (MPI / torchrun style): the one collective of the path on the
 * caller's ncclComm_t (passed as void*), in place on the device block written by iba_eval_*_partial. */
iba_status iba_comm_allreduce(void* nccl_comm, void* d_partials, int32_t B, void* stream);
/* For callers without RCCL headers of their own: communicators over devices of this process (comms[i] belongs to
 * devices[i]; ncclCommInitAll), their rank count, their release. */
iba_status iba_comm_init_all(void** comms, const int32_t* devices, int32_t n);
int32_t iba_comm_count(void* nccl_comm);
iba_status iba_comm_destroy(void* nccl_comm);
/* Which librccl this process runs — "path=<file> runtime=<code> header=<code> match=<0|1>" — and the two version codes
 * (ncclGetVersion of the loaded library, NCCL_VERSION_CODE of the headers this library was compiled against). Inside a
 * torch process the already-mapped torch/lib/librccl.so is the one that is used. */
iba_status iba_rccl_info(char* buf, int32_t cap, int32_t* runtime_version, int32_t* header_version);

/*
 * ---- On-disk formats of the reference pipeline -> problem descriptor [SURVEY.md 8(f) row 1] ----
 * Host-only (no GPU needed). Replaces, for the IBA path, what the reference does with OpenCV/ORB-SLAM2 objects in
 * main(): iba_global.cpp:398-505, iba_local.cpp:325-406, System::RestoreSystemFromFile (System.cc:612-694),
 * KeyFrameConstInfo (KeyFrame.cc:31-80), Map::RestoreMap (Map.cc:162-170), MapPoint(FileNode) (MapPoint.cc:435-451).
 */
typedef struct iba_dataset iba_dataset;
typedef struct iba_dataset_paths {
    const char* frame_id_file;    /* FrameId.yml: "mnId", "mnFrameId" (System.cc:597-609) */
    const char* lidar_pose_file;  /* LOFile: 12 numbers per pose, row-major 3x4 (kitti_tools.h:66-87) */
    const char* pointcloud_dir;   /* KITTI velodyne .bin files; file k (sorted by name, kitti_tools.h:48-62) = frame k */
    const char* keyframe_dir;     /* KeyFrames/NNNNNN.yml written by KeyFrame::saveData (KeyFrame.cc:209-252); the .bin
                                     twins hold only BoW vectors (KeyFrame.h:97-101) and are not read */
    const char* map_file;         /* Map.yml (Map.cc:213-231, MapPoint.cc:454-476) */
    int32_t pointcloud_skip;      /* readPointCloud `skip` (io_tools.h:142-196); iba_global passes 1 (iba_global.cpp:494) */
    int32_t only_positive_x;      /* readPointCloud `only_positive_x`; iba_local passes its config value (iba_local.cpp:394) */
    int32_t num_best_covis;       /* > 0: first N ordered covisible KFs (KeyFrame.cc:417-424); else by weight */
    int32_t min_covis_weight;     /* GetCovisiblesByWeightSafe (KeyFrame.cc:426-439) */
} iba_dataset_paths;

/* Loads and packs a dataset; the descriptor (and everything it points to) lives until iba_dataset_free. */
iba_status iba_dataset_load(const iba_dataset_paths* paths, iba_dataset** out);
const iba_problem_desc* iba_dataset_desc(const iba_dataset* d);
/* mnId / mnFrameId of keyframe f (FrameId.yml order = KeyFrame::lId order) */
iba_status iba_dataset_frame_ids(const iba_dataset* d, int32_t frame, int32_t* mn_id, int32_t* mn_frame_id);
void iba_dataset_free(iba_dataset* d);
/* message of the last failing iba_dataset_* / iba_read_* / iba_write_* call on this thread */
const char* iba_io_last_error(void);

/*
 * The reference's RUN CONFIGURATION (config/calib/NN/iba_calib_global.yml and its iba_func / iba_local siblings): what main()
 * reads with yaml-cpp — the maps io / orb / runtime (iba_global.cpp:412-471, iba_func.cpp:356-406, iba_local.cpp:325-378) — turned
 * into this header's structs, so that a run on the reference pipeline's artefacts takes the reference's own config file.
 * csrc/iba_config.cpp; host only. A missing key is an error (IBA_ERR_IO), as yaml-cpp's .as<T>() throws.
 */
typedef struct iba_run_config iba_run_config;
iba_status iba_run_config_load(const char* yaml_file, iba_run_config** out);
void iba_run_config_free(iba_run_config* c);
const char* iba_run_config_last_error(void);   /* of the last failing iba_run_config_* call on this thread */
/* iba_default_params + the file's runtime keys. local_stage = 0: IBAGlobalParams as iba_global / iba_func fill it
 * (iba_global.cpp:436-459); 1: IBALocalParams as iba_local fills it (iba_local.cpp:358-377). */
iba_status iba_run_config_params(const iba_run_config* c, int32_t local_stage, iba_params* out);
/* The dataset files as main() derives them: BaseDir (+ '/') + VOIdFile / LOFile, PointCloudDir, orb.KeyFrameDir, orb.MapFile,
 * num_best_covis, min_covis_weight. local_stage = 0 ignores PointCloudskip / PointCloudOnlyPositiveX exactly as iba_global does
 * (it reads them and then calls readPointCloud without them, iba_global.cpp:450-451 vs :494); 1 passes them (iba_local.cpp:394).
 * The strings belong to `c` and live until iba_run_config_free. */
iba_status iba_run_config_paths(iba_run_config* c, int32_t local_stage, iba_dataset_paths* out);
/* The NOMAD set-up of the global stage (iba_global.cpp: lb / ub added to x0 :530-533, init_frame, min_mesh, max_bbeval, he_threshold, valid_rate, seed,
 * use_vns) on top of iba_default_mads_options(x0). */
iba_status iba_run_config_mads(const iba_run_config* c, const double* x0, iba_mads_options* out);
/* any entry as text, "section.key" ("io.init_sim3", "runtime.direction_type"; sequences as "[a, b]"); NULL when absent */
const char* iba_run_config_get(const iba_run_config* c, const char* dotted_key);
/* BaseDir (+ '/') + io.<io_key> ("init_sim3", "gt_sim3", "ResFile", "VOFile"); NULL when absent; valid until the next call with the same key */
const char* iba_run_config_path(const iba_run_config* c, const char* io_key);

/* The numbers of one TOP-LEVEL entry of a cv::FileStorage YAML file ("%YAML:1.0": KeyFrames/NNNNNN.yml, Map.yml, ORB-SLAM2 settings
 * such as config/orb_ori/KITTI00-02.yaml, whose Camera.fx.. become KeyFrame::fx..): a scalar, a flow sequence or the data of an
 * !!opencv-matrix node, through the reader iba_dataset_load uses. *n_out = how many there are; at most cap are written. */
iba_status iba_read_cv_yaml_numbers(const char* file, const char* key, double* out, int32_t cap, int32_t* n_out);
/* readPointCloud for .bin (io_tools.h:142-196): XYZI float32 records; with skip > 1 the reference advances its counter
 * by `skip` but reads CONSECUTIVE records, i.e. it keeps the first floor((n - skip) / skip) + 1 points — reproduced.
 * *xyz is malloc'ed (release with iba_io_free). */
iba_status iba_read_kitti_bin(const char* file, int32_t skip, int32_t only_positive_x, float** xyz, int64_t* n_points);
/* ReadPoseList (kitti_tools.h:66-87): complete 12-number records only (the reference additionally appends one junk
 * pose when the file ends with a newline; nothing on the IBA path indexes it). *poses12 is malloc'ed. */
iba_status iba_read_pose_list(const char* file, double** poses12, int64_t* n_poses);
/* readSim3 / writeSim3 (kitti_tools.h:96-158): 12 row-major 3x4 numbers + scale, max_digits10 precision */
iba_status iba_read_sim3(const char* file, double rigid12[12], double* scale);
iba_status iba_write_sim3(const char* file, const double rigid12[12], double scale);
void iba_io_free(void* p);
/* (R, t, s) <-> the 7-vector the evaluators take: x[0:6] = g2o::SE3Quat(R, t).log() (rotation first), x[6] = s raw
 * (iba_global.cpp:511-515, iba_local.cpp:414); inverse = Sim3Exp (g2o_tools.h:105-140). */
iba_status iba_sim3_to_x(const double rigid12[12], double scale, double x[7]);
iba_status iba_x_to_sim3(const double x[7], double rigid12[12], double* scale);

/*
 * ---- Hand-eye initialiser [SURVEY.md 8(f) row 3]: the init_sim3 of the IBA stages without g2o (host only) ----
 * Ta = camera motions (scale-free), Tb = LiDAR motions, each n x 12 (row-major 3x4); result: T_AB (B -> A) and the
 * monocular scale. csrc/iba_handeye.cpp.
 */
iba_status iba_pose_to_motion(const double* poses12, int64_t n, double* motions12 /* (n-1) x 12 */); /* kitti_tools.h:160-165 */
iba_status iba_handeye(const double* Ta12, const double* Tb12, int64_t n, double rigid12[12], double* scale); /* HECalib.h:12-57 */
/* DGHECalib (HECalib.h:66-120), the reference's initialiser for degenerate motion: the rotation as iba_handeye's, translation zero (:109), scale =
 * sum |ta| |tb| / sum |ta|^2 over the pairs whose camera rotation angle is below dg_threshold (reference default 0.01 rad, :66, :82, :112-119;
 * NaN when there is none, as in the reference); *n_degenerate (may be NULL): how many pairs that were. iba_handeye returns IBA_ERR_UNSUPPORTED
 * exactly when its 4 x 4 system is singular — the case this one is for. */
iba_status iba_handeye_degenerate(const double* Ta12, const double* Tb12, int64_t n, double dg_threshold, double rigid12[12], double* scale, int64_t* n_degenerate);
/* The cost HECalibRobustKernelg2o minimises (NLHECalib.hpp:121-163): EdgeHE residual (:27-48), Huber(delta) per pair,
 * optional regulariser on upsilon with information n * ratio; Levenberg-Marquardt with a numerical Jacobian instead of
 * g2o's Dogleg on the reference's hand-written one (see csrc/iba_handeye.cpp). he_calib.cpp: 10 iterations. */
iba_status iba_handeye_robust(const double* Ta12, const double* Tb12, int64_t n, const double rigid12_init[12], double scale_init,
                              double robust_kernel_size, int32_t regulation, double regulation_ratio, int32_t iterations,
                              double rigid12[12], double* scale);
/* HECalibLineProcessg2o (NLHECalib.hpp:189-277): the same residual without a robust kernel but with a per-pair scalar
 * information w^2, w = mu / (mu + chi2), re-estimated between LM solves while mu anneals from mu0 by divid_factor until
 * below min_mu or ex_max_iter outer rounds; the regulariser follows the sum of the weights. The reference ignores its
 * in_max_iter argument and runs 10 inner iterations per solve: pass inner_iterations = 10 for its behaviour. */
iba_status iba_handeye_lineprocess(const double* Ta12, const double* Tb12, int64_t n, const double rigid12_init[12], double scale_init,
                                   int32_t inner_iterations, double mu0, double divid_factor, double min_mu, int32_t ex_max_iter,
                                   int32_t regulation, double regulation_ratio, double rigid12[12], double* scale);

/*
 * ---- ORB-only extrinsic bundle adjustment [SURVEY.md 8(f) row 4] ----
 * One 7-vector vertex x = [rotation vector of R_cl, t_cl, scale] (CalibVertex, Optimizer.cc:40-63: additive update) and
 * N unary reprojection edges (calibEdge, Optimizer.cc:65-205): X_c0 = s * Xw; X_l0 = T_cl^-1 X_c0; X_li = T_lw X_l0;
 * X_ci = T_cl X_li; e = obs - project(X_ci). Per edge: information invSigma2 * I, Huber(sqrt(5.991)).
 * The device evaluates every edge (residual, Jacobian by forward-mode duals exactly as g2o's auto-diff does, robust
 * weight; one expression is rearranged: 1 - cos(theta) of the angle-axis block is sin^2 / (1 + cos) where cos > 0, so that the
 * Jacobian keeps its digits at a small non-zero rotation) and reduces the normal equations; the host runs g2o's Levenberg-Marquardt and the reference's four
 * optimise / classify rounds (Optimizer.cc:1511-1556 = 1698-1743). csrc/iba_ba.hip.
 */
typedef struct iba_ba_handle iba_ba_handle;
typedef struct iba_ba_desc {
    int64_t n_edges;
    int32_t n_frames;
    const double* frame_Tlw6;   /* [F*6] e->Tlw_quat: rotation vector and translation (Optimizer.cc:1457-1462 / 1627-1632) */
    const double* frame_intr;   /* [F*4] fx, fy, cx, cy */
    const int32_t* edge_frame;  /* [N] */
    const double* edge_Xw;      /* [N*3] e->Xw (the MapPoint in the reference camera frame, CV_32F values widened) */
    const double* edge_obs;     /* [N*2] kpUn.pt */
    const double* edge_info;    /* [N] invSigma2 = mvInvLevelSigma2[octave] */
    const int32_t* edge_slot;   /* [N] vnIndexEdgeMono: MapPoint slot inside its keyframe — the reference indexes its
                                   outlier flags with it, so flags alias across keyframes (reproduced). NULL = the edge's own
                                   index; every slot must be >= 0 (iba_ba_create answers IBA_ERR_INVALID_ARG otherwise) */
} iba_ba_desc;
typedef struct iba_ba_result {
    double x[7];
    int32_t n_inliers;          /* nInitialCorrespondences - nBad */
    int32_t n_edges;
    int32_t lm_iterations;      /* over the four rounds */
    int32_t evaluations;        /* device evaluations of the edge set */
    double chi2[4];             /* robustified chi2 of the active edges at the end of each round */
    int32_t n_bad[4];
} iba_ba_result;
iba_status iba_ba_create(const iba_ba_desc* desc, int device, iba_ba_handle** out);
void iba_ba_destroy(iba_ba_handle* h);
const char* iba_ba_last_error(const iba_ba_handle* h);
/* One linearisation at x: H (49, row-major, symmetric), b (7) and the robustified chi2 summed over the edges with
 * active[i] != 0 (NULL = all); robust = 0 drops the Huber kernel (round 4 of the reference). chi2_edges (NULL or [N])
 * receives e^T Omega e of EVERY edge. Sign convention of g2o: solve (H + lambda I) dx = b, x += dx. */
iba_status iba_ba_eval(iba_ba_handle* h, const double* x, const uint8_t* active, int32_t robust, double* H, double* b,
                       double* chi2_robust, double* chi2_edges);
/* OptimizeExtrinsicGlobal / OptimizeExtrinsicLocal schedule on the edge list (which of the two it is depends only on how
 * Xw and Tlw6 were built): 4 x (reset to x0, 10 LM iterations, classify at chi2 > 5.991), kernel off after round 3. */
iba_status iba_ba_optimize(iba_ba_handle* h, const double* x0, iba_ba_result* res);

/* Edge list of the ORB-only extrinsic BA straight from the dataset directory; LiDAR poses as ba_calib.cpp:43-44 passes them.
 * global = 1: OptimizeExtrinsicGlobal constants (Optimizer.cc:1611-1676); global = 0: OptimizeExtrinsicLocal (:1437-1501: MapPoints
 * in the frame of the oldest of the 20 best covisible keyframes, LiDAR pose relative to it). */
typedef struct iba_ba_dataset iba_ba_dataset;
iba_status iba_dataset_load_ba(const iba_dataset_paths* paths, int32_t global, iba_ba_dataset** out);
const iba_ba_desc* iba_ba_dataset_desc(const iba_ba_dataset* d);
void iba_ba_dataset_free(iba_ba_dataset* d);

#ifdef __cplusplus
}
#endif
#endif /* IBA_MI355X_H */
