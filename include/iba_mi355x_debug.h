/*
 * iba_mi355x_debug.h — diagnostics of the MI355X IBA evaluation path: timing probes, counters, the kernels' own searches and
 * plane fits exposed for parity tests, and the host-only self-tests of the optimiser logic. Test and benchmark tooling; none of
 * it is part of the drop-in surface (iba_mi355x.h), none of it changes a result, and an integrator never needs it.
 *
 * DEBUG-ONLY ENVIRONMENT VARIABLES (read at iba_create / iba_group_create, AND ONLY WHEN IBA_DEBUG_ENV=1 IS SET AS WELL — round 6: a stray
 * variable in an integrator's environment changes nothing; an integrator sets iba_create_options instead — where a variable has a field
 * there, the FIELD is the interface and the variable only overrides it for A/B runs of an unmodified caller):
 *
 *   variable                field of iba_create_options   meaning
 *   IBA_COMMON_PAIRS        common_pairs                  0 never share the 2d-3d pair search, 1 when tight, 2 always
 *   IBA_COMMON_MAX_PX       common_max_px                 nominal spread (px) up to which a batch shares one pair search
 *   IBA_PAIR_GROUPS         max_pair_groups               clustering of a wide batch into 1..4 tight groups
 *   IBA_PAIR_MEMO           pair_memo                     reuse of pair lists across calls
 *   IBA_PAIR_MEMO_MAX_B     pair_memo_max_batch           largest batch whose lists are built reusable
 *   IBA_PAIR_INFL           pair_inflation                inflation of a reusable list's bound
 *   IBA_NN_SETS             anchored_lists                anchored neighbour lists on / off
 *   IBA_ANCHOR_REACH        anchor_reach                  drift (m) that moves an anchor
 *   IBA_SPIN_WAIT           spin_wait                     polling wait at the end of a call
 *   IBA_FACTOR_MFMA         factor_mfma                   normal-equation sums on the matrix cores
 *   IBA_DEBUG_PAIR_CAP      pair_list_capacity            entries per pair list (tests force the overflow path)
 *   IBA_CHAIN_FOLD          chain_fold                    staging / reduction launches folded into their neighbours
 *   IBA_MAX_CHAIN           max_chain_batch               candidates one launch chain takes
 *   -- no field: pure diagnostics, results unaffected unless stated --
 *   IBA_NN_CG, IBA_PAIRS_DENSE_MIN, IBA_PAIRS_WAVE (the pair search's form: iba_debug_last_pairs_threads), IBA_COMMON_MIN_BATCH, IBA_PAIR_BOUND, IBA_ASSOC2_FLREG, IBA_ASSOC2_THREADS (256 / 512 threads per
 *   block of the shared-pair association, else chosen per launch), IBA_ASSOC2_SMALL_MIN, IBA_ASSOC_BLOCKS, IBA_CAND_BYTES,
 *   IBA_PAIR_BYTES                                        launch-shape / LDS-plan knobs of single kernels (A/B timing)
 *   IBA_PAIRS_VISIBLE                                     0: the pair search always runs its full (chunks, keyframes) grid, never the visible-chunk list (iba_debug_pairs_visible)
 *   IBA_NN_ROUNDS                                         0: the entries the anchored lists leave over are searched leaf by leaf (rounds 3-4) instead of
 *                                                         in rounds of leaves (same results; A/B timing)
 *   IBA_DONE_FLAG                                         0: a blocking call polls its stream (rounds 3-4) instead of the sequence number the summing
 *                                                         kernel's last block publishes in pinned memory (same results; A/B timing)
 *   IBA_NN_SMALL, IBA_NN_SMALL_MIN_B                      0 / 1: the search kernel in blocks of four waves / of one wave whatever the size of the kd trees; from how many candidates per launch
 *   IBA_NN_LIST                                           1: the anchored lists are walked by the persistent list kernel, measured slower: csrc/iba_nn_list_kernel.hpp;
 *                                                         IBA_NN_LIST_WORKERS=n: its blocks per CU
 *   IBA_FACTOR_V2                                         1: the normal equations by iba_factor2_kernel — one wave per equal share of a candidate's whole work
 *                                                         list (csrc/iba_factor2_kernel.hpp) — instead of one wave per (keyframe, candidate); same sums to
 *                                                         summation order, measured no faster; IBA_FACTOR_WAVES_PER_CAND forces its ranges per candidate
 *   IBA_NN_DBG, IBA_ASSOC_DBG, IBA_FACTOR_DBG             cut a kernel short after a phase (timing attribution; RESULTS ARE GARBAGE)
 *   IBA_LAYOUT_DEBUG, IBA_DEBUG_LEFT_HIST                 print the LDS plan / a histogram of left-over searches to stderr
 *   IBA_GROUP_TIMEOUT_MS                                  bound (ms, default 20 000; x4 for a group's first call) of a device thread's
 *                                                         wait for its stream before the group is declared broken
 *   IBA_PGO_MAX_SEP                                       the separator cap of iba_pgo_create / iba_pgo_plan in place of IBA_PGO_MAX_SEPARATORS (1 .. 1024; tests reach
 *                                                         the doubling of K at a small graph)
 *   IBA_PROJECT_BUDGET                                    bytes a chunk of iba_project_run's jobs may take (key, depth and index images: 16 per pixel and job) in
 *                                                         place of IBA_PROJECT_BUDGET_BYTES and the free-memory rule, read at every call (tests reach the
 *                                                         split of a call at small images; same results)
 *   IBA_PROJECT_TIMING                                    set: iba_project_run and the colourise / overlay accessors record HIP events around their kernels
 *                                                         (iba_debug_projection_kernel_ms; tools/project_bench.py); same results
 *   IBA_ORB_BUDGET, IBA_ORB_TIMING                        the same two for iba_orb_extract (6 bytes per pyramid pixel and image; iba_debug_orb_chunks,
 *                                                         iba_debug_orb_stage_ms; tools/orb_bench.py); same results
 *   IBA_ORB_MATCH_BUDGET, IBA_ORB_MATCH_TIMING            the same two for iba_orb_match (6 bytes per candidate-list entry; iba_debug_orb_match_chunks,
 *                                                         iba_debug_orb_match_stage_ms; tools/orb_match_bench.py); same results
 *   IBA_TWOVIEW_BUDGET, IBA_TWOVIEW_TIMING                the same two for iba_twoview_init (187 bytes per match and 148 per iteration of a pair; iba_debug_twoview_chunks, iba_debug_twoview_stage_ms;
 *                                                         tools/twoview_bench.py); same results
 *   IBA_POSE_BUDGET, IBA_POSE_ONCHIP, IBA_POSE_TIMING     iba_pose_optimize / iba_pose_eval: the bytes a chunk of jobs may take on the device in place of 1 GiB
 *                                                         (iba_debug_pose_chunks), an on-chip edge capacity below IBA_POSE_ONCHIP_EDGES, and HIP events around
 *                                                         the kernel (iba_debug_pose_kernel_ms; tools/pose_bench.py); same results
 *   IBA_BUNDLE_BUDGET, IBA_BUNDLE_TIMING                  iba_bundle_optimize / iba_bundle_eval: the bytes a chunk of jobs may take on the device in place of 1 GiB
 *                                                         (iba_debug_bundle_chunks) and HIP events around a chunk's launch chains
 *                                                         (iba_debug_bundle_kernel_ms; tools/bundle_bench.py); same results
 *   IBA_MAP_MATCH_BUDGET, IBA_MAP_MATCH_TIMING            iba_map_match: the bytes a chunk's candidate lists may take (6 per entry) in place of 1 GiB and the
 *                                                         free-memory rule (iba_debug_map_match_chunks), and HIP events around the stages
 *                                                         (iba_debug_map_match_stage_ms; tools/map_match_bench.py); same results
 *   IBA_TRIANGULATE_BUDGET, IBA_TRIANGULATE_TIMING        the same two for iba_triangulate (120 bytes per (neighbour, keypoint) slot; iba_debug_triangulate_chunks,
 *                                                         iba_debug_triangulate_stage_ms; tools/triangulate_bench.py); same results
 *   IBA_TRIANGULATE_PICK_LANES                            8 / 16 / 64: the lanes per query of iba_triangulate's pick kernel in place of the shipped width
 *                                                         (same results; A/B timing and the tests of all three)
 *   IBA_FUSE_BUDGET, IBA_FUSE_TIMING                      the same two for iba_fuse (6 bytes per candidate-list entry; iba_debug_fuse_chunks,
 *                                                         iba_debug_fuse_stage_ms; tools/fuse_bench.py); same results
 *   IBA_FUSE_PICK_LANES                                   8 / 16 / 64: the lanes per slot of iba_fuse's pick kernel in place of the shipped width
 *                                                         (same results; A/B timing and the tests of all three)
 *   IBA_REFRESH_TIMING                                    iba_refresh records HIP events around its three launches (iba_debug_refresh_stage_ms;
 *                                                         tools/refresh_bench.py); same results
 *   IBA_REFRESH_NARROW_LANES                              4 / 8 / 16 / 32: the lanes per point of iba_refresh's narrow shape in place of the shipped
 *                                                         width (same results; A/B timing and the tests of all four)
 *   IBA_REFRESH_MEDIAN                                    0: the binary search that recomputes a row's distances; 1: one pass that keeps the row (same
 *                                                         results; A/B timing and the tests of both)
 *   IBA_REFRESH_MIN_PATH                                  1 / 2: no listed point of iba_refresh takes a shape below the wave / the block shape (same
 *                                                         results; the tests that run a whole scene on each wider shape)
 *   IBA_SIM3_TIMING                                       iba_sim3_solve records HIP events around its five stages (iba_debug_sim3_stage_ms;
 *                                                         tools/sim3_bench.py); same results
 *   IBA_SIM3_COUNT_FORM                                   0 / 1: form (a), a lane per hypothesis, or form (b), a lane per correspondence, of
 *                                                         iba_sim3_solve's count kernel in place of the shipped one (same results; A/B timing and
 *                                                         the tests of both)
 *   IBA_SIM3_BUDGET                                       the chunk budget of iba_sim3_solve in bytes in place of IBA_SIM3_BUDGET_BYTES (same results;
 *                                                         the tests that cut a call into several chunks)
 *   IBA_GROUP_REDUCE_HOST (flag of iba_group_create_ex, not a variable), IBA_DEBUG_FAIL_RANK / IBA_DEBUG_FAIL_PHASE: inject one
 *                                                         failure into a group's evaluation (tests of the fail-not-hang path)
 */
#ifndef IBA_MI355X_DEBUG_H
#define IBA_MI355X_DEBUG_H

#include "iba_mi355x.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Introspection for benchmarks: device-side duration of the last evaluation's dominant kernel
 * measured with HIP events on the launch stream (ms), and the frame-kernel launch shape. */
iba_status iba_last_kernel_ms(iba_handle* h, float* frame_kernel_ms, float* total_ms);
iba_status iba_set_timing(iba_handle* h, int32_t enable);
/* the same split by kernel: association kernel (projection, 2d-3d association, 3d-2d residuals), grouped 1-NN search kernel
 * (3d-3d terms), and everything after them (factor kernel, sums) */
iba_status iba_last_phase_ms(iba_handle* h, float* assoc_kernel_ms, float* nn_kernel_ms, float* rest_ms);
/* debug (library built with -DIBA_DIAG_COUNTERS only, `make -C csrc diag`; zeros otherwise): cycle sums per phase of the search kernel (thread 0 of every block:
 * start-up, entries + MapPoints, list rows, picks, wait at the end of the list pass, left-over searches, sums) and the number of blocks */
iba_status iba_debug_phase_cycles(iba_handle* h, uint64_t out8[8], int32_t reset);
iba_status iba_debug_phase_cycles12(iba_handle* h, uint64_t out12[12], int32_t reset);   /* the same with iba_nn_list_kernel's four slots inside its picks */
/* debug: threads per block of the last iba_assoc2_kernel launch on this handle (256 or 512: chosen per launch from the number of (candidate,
 * keyframe) blocks; 0 = no shared-pair association has run) */
int32_t iba_debug_last_assoc2_threads(const iba_handle* h);
/* debug: ranges per candidate iba_factor2_kernel would cut a batch of B into on this handle; 0 = the batch runs on the one-wave-per-(keyframe,
 * candidate) factor kernel (the default) */
int32_t iba_debug_factor_ranges(const iba_handle* h, int32_t B);
/* debug: host copy of the summed partial blocks of the last iba_eval_* call */
iba_status iba_debug_last_partials(iba_handle* h, double* out, int32_t B);
/* debug: which 2d-3d association ran in the last evaluation chain: 1 = the batch shared one pair search per keyframe
 * (any batch, a single candidate included, whose nominal projection spread stays under IBA_COMMON_MAX_PX = 20 px), 0 = every
 * candidate searched for itself. The results are the same bits either way.
 * Environment (read at iba_create): IBA_COMMON_PAIRS=0 never share, 2 share whenever the bound allows; IBA_COMMON_MAX_PX;
 * IBA_PAIR_MEMO=0 no reuse of pair lists across calls, IBA_PAIR_MEMO_MAX_B (40) the largest batch that reuses, IBA_PAIR_INFL (1.25)
 * the inflation of a reusable list's bound; IBA_SIDE_STREAM=0 one stream only; IBA_SPIN_WAIT=0 blocking waits. */
int32_t iba_debug_last_path(const iba_handle* h);   /* 2: the batch was clustered into several tight groups with one pair search each */
/* The planner behind that decision on B <= IBA_MAX_BATCH candidates, host only (no GPU): a batch whose nominal projection spread
 * (at a point 12 m out, 10 m deep, focal length max_fx) exceeds max_px is clustered into at most max_groups (<= 4) groups, accepted
 * when every group is within max_px. group_of[B] (may be NULL) receives each candidate's group, group_px[4] (may be NULL) the
 * groups' nominal spreads, *n_groups 1 (one shared search), 2..4 (clustered) or 0 (wide everywhere: every candidate for itself). */
iba_status iba_debug_plan_groups(const double* x, int32_t B, double max_fx, double max_px, int32_t max_groups, int32_t* group_of, double* group_px, int32_t* n_groups);
/* debug: how often the anchored neighbour lists (the 1-NN search memoised around an anchor extrinsic that follows the
 * optimiser's candidates; IBA_NN_SETS=0 disables them, IBA_ANCHOR_REACH sets the drift in metres that moves the anchor) have
 * been built on this handle. Results do not depend on the anchor: every lane certifies its pick or searches the tree. */
int32_t iba_debug_anchor_builds(const iba_handle* h);
/* diagnostic: how many times the shared pair search has run on this handle (an evaluation whose batch stays inside the bound of
 * the lists an earlier call built reuses them: IBA_PAIR_MEMO, default on) */
int32_t iba_debug_pairs_builds(const iba_handle* h);
/* debug: the form of the last shared pair search: 64 / 256 / 512 = one wave per 64-position culling chunk in blocks of that many
 * threads (the default, 64, while the scans are below pairs_dense_min points), 0 = the 512-thread block kernel (the default on
 * dense scans); -1 before any. IBA_PAIRS_WAVE=0 / 64 / 256 / 512 forces a form. Same results whichever form runs. */
int32_t iba_debug_last_pairs_threads(const iba_handle* h);
/* debug: the (scan point, keypoint) pair list of (list slot, local frame) that the last pair search left: out_pairs[2 i] = original
 * scan point index, out_pairs[2 i + 1] = keypoint id, in list order (which varies from run to run); at most cap entries are copied.
 * slot -1: the slot of the last call's first group. Returns the length of the list (capped at the list capacity), -1 on a bad argument.
 * The list is a superset of the pairs any candidate of the batch can accept (see iba_pairs_kernel). */
int32_t iba_debug_pair_list(iba_handle* h, int32_t slot, int32_t frame, uint32_t* out_pairs, int32_t cap);
/* debug: the visible-chunk list of the shared pair search (one wave per listed 64-position chunk — one block per listed run of eight chunks in the
 * 512-thread form — instead of one per chunk of every scan; built around an anchor transform with an entrywise bound, rebuilt when a batch leaves
 * the bound. A rebuild is launched behind the call that found the batch outside and waits for nothing: that call runs the full grid, the next
 * search walks the new list. IBA_PAIRS_VISIBLE=0 forces the full grid.
 * out4 = {items in the list (0: none ready), rebuilds so far, 1 if the last pair search walked the list, items a full grid has}. Same results
 * with or without the list: every wave still tests its chunk against the call's own bound. */
iba_status iba_debug_pairs_visible(const iba_handle* h, int32_t out4[4]);
/* debug: the bound a rebuild of that list is given — the batch's own bound times infl (>= 1) plus the floors (rotation entries >= 1e-3, metres
 * >= 1e-2) — and the least number of pair searches between two rebuilds (defaults 4, 1e-3, 1e-2, 4; tools/vis_sweep.py) */
iba_status iba_debug_set_pairs_visible_bound(iba_handle* h, double infl, double rho_floor, double tau_floor, int32_t gap);
/* debug (host arithmetic, no GPU): the chunk test of the pair kernels and of the list builder, the same function compiled for the host. g24: R[9],
 * t[3], rho[9], tau[3]; box8: min xyz, -, max xyz, -; cam5: fx, cx, cy, W, H. 1: no transform within the bound sees the box, 0: kept */
int32_t iba_debug_chunk_box_culled(const double g24[24], const float box8[8], const double cam5[5]);
/* debug: how many chunks pass the pair search's chunk test under the bound of group `group` of the LAST pair search (the first chunk of a
 * keyframe always counts: it clears counters); waits for the stream. -1 on a bad argument or when no pair search has run. */
int64_t iba_debug_pairs_chunks_passing(iba_handle* h, int32_t group);
/* debug (host only): the composition rule of that list — the entrywise bound (out12: rho[9], tau[3]) around the anchor (Ra, ta) of every
 * transform within (rho_g, tau_g) of the group reference (Rg, tg) */
iba_status iba_debug_vis_compose(const double Ra[9], const double ta[3], const double Rg[9], const double tg[3], const double rho_g[9], const double tau_g[3], double out12[12]);
/* debug (host only): the check a call makes before it walks the list: 1 when the group (Rg, tg, rho_g, tau_g) lies inside (rho_a, tau_a) around the anchor */
int32_t iba_debug_vis_covers(const double Ra[9], const double ta[3], const double rho_a[9], const double tau_a[3], const double Rg[9], const double tg[3], const double rho_g[9], const double tau_g[3]);
/* diagnostic: list entries of the last evaluation (all candidates) that the anchored neighbour lists could not settle and the
 * tree search took over; -1 when no search ran */
double iba_debug_nn_left_to_tree(iba_handle* h);
int32_t iba_debug_last_nn_threads(const iba_handle* h);   /* threads per block of the last search launch: 64 = one-wave blocks (small kd trees, 12 candidates or more), 256 otherwise */
int32_t iba_debug_last_nn_list(const iba_handle* h);   /* > 0: the last search launch was the opt-in persistent list kernel, IBA_NN_LIST=1, with that many workers per XCD and group */
/* diagnostic: mean number of (scan point, keypoint) pairs per keyframe that the last shared pair search listed; -1: none ran */
double iba_debug_mean_pairs(iba_handle* h);
/* debug (host only): R[9], t[3], dR/d omega_k [3][9], dt/dx_k [6][3], s of a candidate as the factor kernel reads them (58 doubles) */
iba_status iba_debug_cand(const double x[7], double out58[58]);
/* debug: association blocks since the last reset that rescanned every scan point (a speed-only fallback: full queue / pair list) */
int64_t iba_debug_rescans(iba_handle* h, int32_t reset);
/* debug: out4 = {those rescans, iba_assoc2_kernel blocks whose note list of possible winners overflowed (speed only), 0, 0} since the last reset */
iba_status iba_debug_counters(iba_handle* h, uint32_t out4[4], int32_t reset);
/* debug: {pair lists of the last call that had overflowed (their blocks rescan every point: speed only), lists read, longest list} */
iba_status iba_debug_pair_lists(iba_handle* h, int32_t out3[3]);
/* debug: exact 1-NN (nanoflann semantics with the lowest-index tie rule, iba_global.cpp:116-122) of n LiDAR-frame query
 * points in the scan of local frame `frame`, run through the search kernel's own kd search, one lane per query: original point
 * index and exact squared distance. mode 1: as the association path's query alone; 2: as the cost path's alone; 3 / 4: both paths
 * searched together as the kernel does, the query as the first (3) or the second (4) with its partner 1e-7 beside it.
 * For parity tests of the search itself. */
iba_status iba_debug_nn(iba_handle* h, int32_t frame, const double* q_xyz, int32_t n, int32_t mode, uint32_t* out_idx, double* out_d2);
/* debug: the memoised local plane (plane_cache = 1) at scan point `point` (ORIGINAL index) of owned frame `frame`: which = 0 the cost
 * path's planes (norm_radius / norm_max_pts), 1 the association / Jacobian path's (neigh_radius / neigh_max_pts). With plane_cache = 0
 * only which = 1 after iba_build_problem: the plane the frozen problem's residual blocks read (fitted where a block needed one; other
 * points hold stale records). out5 = unit normal
 * (3), sum of |(p_i - c) . n|, squared distance of the farthest kept neighbour; *k = kept neighbours. The parity tests substitute this
 * normal into the oracle's residual block: the device fits planes with its own libm, and an ill-conditioned block amplifies the
 * last-bit difference of the two normals (tests/parity_explain.py). */
iba_status iba_debug_plane(iba_handle* h, int32_t frame, uint32_t point, int32_t which, double out5[5], int32_t* k);
/* debug: force the block shape of iba_scan_* passes (64: one-wave blocks, 256: four waves; 0: the rule of DESIGN.md 5b on the largest target
 * tree of the pass). The sums do not depend on the shape. iba_debug_last_scan_threads: the shape the last pass ran with. */
/* debug: the scan-side index of local frame `frame` as the kernels read it, on any handle: perm (tree position -> original index), the points in
 * tree order as three planes x[P], y[P], z[P], the inner nodes in heap order ((1 << depth) - 1 each), the boxes of the 64-position chunks (8
 * floats each: min xyz, NaN, max xyz, the largest |coordinate|), the frame's box, the depth. Every output may be NULL; P = iba_frame_num_points.
 * tests/test_gpu_submap_handle.py holds the device-built index of iba_submap_handle to the host-built one of iba_create with it, byte for byte. */
iba_status iba_debug_scan_index(iba_handle* h, int32_t frame, uint32_t* perm /* P */, float* xyz_tree /* 3 x P, tree order */,
                                uint32_t* node_dim, float* node_split /* (1<<depth)-1 each */, float* chunk_box /* 8 per chunk */,
                                float frame_box[8], int32_t* depth);
/* debug, HOST ONLY (no device is touched): the host build of the same index (build_tree, csrc/iba_build.hpp) on P points given as x, y, z triples:
 * perm, the nodes, the depth. tests/test_index_rules_cpu.py pins the numpy restatement of the build rules to it. */
iba_status iba_debug_build_tree(const float* xyz, uint32_t P, uint32_t* perm, uint32_t* node_dim, float* node_split, int32_t* depth);
iba_status iba_debug_scan_threads(iba_handle* h, int32_t threads);
int32_t iba_debug_last_scan_threads(const iba_handle* h);

/* the same driver on built-in analytic black boxes (host only; for tests of the search logic without a GPU):
 * 0 smooth bowl, 1 bowl with an active constraint and an infeasible start, 2 nonsmooth with two constraints,
 * 3 shallow bowl covered with narrow local basins (for the variable-neighbourhood restarts) */
iba_status iba_mads_selftest(int32_t problem, const double* x0, const iba_mads_options* opt, iba_mads_result* res);
/* the same two calls with the sequence of black-box evaluations recorded: `trace` receives up to `cap` rows of 8 doubles
 * (x[7], f) in evaluation order, *n_trace the number of evaluations (tests diff the sequence against oracle/mads.py) */
iba_status iba_calibrate_mads_trace(iba_handle* h, const double* x0, const iba_mads_options* opt, iba_mads_result* res, double* trace, int32_t cap, int32_t* n_trace);
/* ... and with the black-box CALLS recorded as well: batch_sizes receives up to cap_batches call sizes in order (they split the
 * rows of `trace` into the batches iba_eval_bbo was given), *n_batches their number. bench.py replays such a record through
 * iba_eval_bbo (extras.mads_trace_replay). */
iba_status iba_calibrate_mads_record(iba_handle* h, const double* x0, const iba_mads_options* opt, iba_mads_result* res, double* trace, int32_t cap, int32_t* n_trace,
                                     int32_t* batch_sizes, int32_t cap_batches, int32_t* n_batches);
iba_status iba_mads_selftest_trace(int32_t problem, const double* x0, const iba_mads_options* opt, iba_mads_result* res, double* trace, int32_t cap, int32_t* n_trace);


/* debug: the sorted neighbour lists of the plane fits — the list builder of the plane kernels, i.e. ComputeAlignmentDist's
 * kNN(norm_max_pts) around nn_pt (iba_global.cpp:125-133; ComputeLocalNeighbor, pointcloud.h:733-760) — around n scan points (ORIGINAL
 * indices) of owned frame `frame`: up to k <= 64 neighbours with d^2 < r2 each (INFINITY: no clip), nearest first, the point itself
 * first at distance 0. out_idx / out_d2 are n x k (0xFFFFFFFF / -1 beyond out_cnt[i]). Equal distances keep the visiting order of THIS
 * library's tree (nanoflann keeps its own tree's): only exact ties can differ from the reference's lists. */
iba_status iba_debug_knn(iba_handle* h, int32_t frame, const uint32_t* points, int32_t n, int32_t k, double r2, uint32_t* out_idx, double* out_d2, int32_t* out_cnt);

/* debug: what a blocking entry point costs a C caller (no language binding in the clock): `iters` back-to-back calls — after three that do not
 * count — of iba_eval_cost (kind 0), iba_eval_full (kind 1) or iba_eval_factors (kind 2; needs iba_build_problem) on the same B candidates, each
 * timed here with the steady clock. *median_ms, *min_ms (may be NULL) per call. The unmodified caller of the reference is such a loop
 * (BALoss::eval_x, iba_global.cpp:385: one candidate per call). */
iba_status iba_debug_call_latency(iba_handle* h, const double* x, int32_t B, int32_t kind, int32_t iters, double* median_ms, double* min_ms);

/* debug: the kernels' shared-reciprocal division (two quotients by one depth: csrc/iba_kernels.hpp, div2) beside the compiler's IEEE f64
 * division, on n operand triples from the caller, on `device`. q0/q1 = num0/den, num1/den as the projections compute them, ref0/ref1 = as
 * the plain division does; *n_fast = triples that took the shared-reciprocal path (the others fall back to the plain division inside). The
 * two must agree bit for bit on every operand (tests/test_gpu_division.py; iba_global.cpp:70-75, :308-313 are the divisions they stand for). */
iba_status iba_debug_div2_selftest(int32_t device, const double* num0, const double* num1, const double* den, int64_t n, double* q0, double* q1, double* ref0, double* ref1, int64_t* n_fast);

/* debug: the LM trials of the last iba_pgo_optimize in order, one byte each: 1 accepted, 0 rejected, 2 the trial that stopped on the increment; bit 7
 * set on the trials of pass 2. Up to cap bytes are written; *n = the number of trials. */
iba_status iba_debug_pgo_trace(iba_pgo* pg, uint8_t* trials, int32_t cap, int32_t* n);

/* debug: the LM trials of the last iba_smooth_update in order, one byte each: 1 accepted, 0 rejected, 2 the trial that stopped on the increment. Up to
 * cap bytes are written; *n = the number of trials. */
iba_status iba_debug_smooth_trace(iba_smooth* s, uint8_t* trials, int32_t cap, int32_t* n);

/* debug, host only (no device): the argument checks of iba_project_run on a stand-in for the handle — n_frames local frames with intrinsics6
 * (n_frames x 6: fx, fy, cx, cy, W, H), NULL for a scans-only handle. The status and message (iba_project_last_error) iba_project_run would give. */
iba_status iba_debug_project_validate(int32_t n_frames, const double* intrinsics6, const double* x7, const int32_t* frames, int32_t J, const iba_project_options* opt);
/* debug, host only: a result of n_jobs empty jobs without device buffers (the accessors' job-index checks); release it with iba_projection_free. */
iba_status iba_debug_project_stub(int32_t n_jobs, iba_projection** out);
/* debug: the chunks the jobs of the call behind p were cut into (IBA_PROJECT_BUDGET); 0 for NULL */
int32_t iba_debug_projection_chunks(const iba_projection* p);
/* debug: with IBA_PROJECT_TIMING set at the call, HIP-event times (ms) of the kernels behind p: [0] splat, [1] resolve, [2] visible, each summed over
 * the chunks of iba_project_run; [3] the last iba_projection_colorize's launch, [4] the last iba_projection_overlay's. Zeros without the variable. */
iba_status iba_debug_projection_kernel_ms(const iba_projection* p, float ms[5]);

/* debug, host only: O7's degree arctangent polynomial and O9's pair for one angle in degrees: ab = (a, b) = (cos, sin) rounded to float as the
 * descriptor kernel uses them, cs = the f64 cosine and sine before the rounding (iba_orb_* of iba_mi355x.h; the functions are compiled once for host
 * and device, csrc/iba_orb_host.hpp) */
float iba_debug_orb_atan2(float y, float x);
iba_status iba_debug_orb_sincos(float angle_deg, float ab[2], double cs[2]);
/* debug, host only: a result of n_images empty images without device buffers (the accessors' index and keep_stages checks); release it with iba_orb_free */
iba_status iba_debug_orb_stub(int32_t n_images, int32_t n_levels, int32_t keep_stages, iba_orb_features** out);
/* debug: the chunks the images of the call behind f were cut into (IBA_ORB_BUDGET: bytes a chunk may take in place of IBA_ORB_BUDGET_BYTES and the
 * free-memory rule, read at every call under IBA_DEBUG_ENV=1; same results); 0 for NULL */
int32_t iba_debug_orb_chunks(const iba_orb_features* f);
/* debug: with IBA_ORB_TIMING set at the call (under IBA_DEBUG_ENV=1), times in ms summed over the chunks: [0] resize, [1] score, [2] cell count + scan +
 * write, [3] the host's share between them and the next launch (both candidate copies, O6, the keypoints up; steady clock), [4] orientation, [5] blur,
 * [6] descriptor; the kernels' from HIP events. Zeros without the variable. Same results. */
iba_status iba_debug_orb_stage_ms(const iba_orb_features* f, float ms[7]);
/* debug: O8 and O9 alone on one image taken as a level: the blurred image (may be NULL) and the descriptors of n keypoints at given level pixels
 * (>= 19 from every edge) and given angles in degrees. Tests reach the rint ties of O9 with it, which no image reaches on purpose. */
iba_status iba_debug_orb_describe(const uint8_t* gray, int32_t W, int32_t H, const int32_t* xy, const float* angle, int32_t n, const int8_t* pattern, int device, uint8_t* blurred, uint8_t* desc);
/* debug, host only: a result of n_jobs jobs without queries over n_frames frames without keypoints (the accessors' index and keep_stages checks);
 * release it with iba_orb_matches_free */
iba_status iba_debug_orb_match_stub(int32_t n_jobs, int32_t n_frames, int32_t keep_stages, iba_orb_matches** out);
/* debug: the chunks the jobs of the call behind m were cut into (IBA_ORB_MATCH_BUDGET: bytes a chunk's candidate lists may take in place of
 * IBA_ORB_MATCH_BUDGET_BYTES and the free-memory rule, read at every call under IBA_DEBUG_ENV=1; same results); 0 for NULL */
int32_t iba_debug_orb_match_chunks(const iba_orb_matches* m);
/* debug: with IBA_ORB_MATCH_TIMING set at the call (under IBA_DEBUG_ENV=1), times in ms from HIP events, summed over the chunks: [0] grid (cell, scan,
 * fill), [1] list count, [2] scan + list write with the distances, [3] resolve. Zeros without the variable. Same results. */
iba_status iba_debug_orb_match_stage_ms(const iba_orb_matches* m, float ms[4]);
/* debug, host only: the chunk planner on its own: the cut of n_jobs jobs with the given candidate counts under budget bytes; cut receives *n_cut
 * <= n_jobs + 1 ascending job indices, the first 0 and the last n_jobs */
iba_status iba_debug_orb_match_plan(const int64_t* candidates, int32_t n_jobs, uint64_t budget, int32_t* cut, int32_t* n_cut);
/* debug, host only: the whole of iba_twoview_init through the host restatement of its rules (csrc/iba_twoview_host.hpp over the arithmetic the
 * kernels compile, csrc/iba_twoview_math.hpp), no device; the same checks, the same result object and accessors */
iba_status iba_debug_twoview_host(const iba_twoview_pair* pairs, int32_t B, const iba_twoview_options* opt, iba_twoview_batch** out);
/* debug, host only: rule T2 on its own on a row-major float32 matrix of 16 x 9, 8 x 9, 4 x 4 or 3 x 3: v takes n entries, *sweeps the sweeps
 * that rotated (30: the cap was reached); v64 (n entries, may be NULL) the float64 column v was rounded from */
iba_status iba_debug_twoview_null_vector(const float* A, int32_t m, int32_t n, float* v, double* v64, int32_t* sweeps);
/* debug: the null-vector solves of the call behind r whose 30th sweep still rotated; 0 for NULL */
int32_t iba_debug_twoview_sweep_cap_hits(const iba_twoview_batch* r);
/* debug: the chunks the call behind r ran as (a chunk none of whose pairs has 8 matches counts too); 0 for iba_debug_twoview_host and for NULL */
int32_t iba_debug_twoview_chunks(const iba_twoview_batch* r);
/* debug: with IBA_TWOVIEW_TIMING set at the call (under IBA_DEBUG_ENV=1), times in ms from HIP events, summed over the chunks: [0] hypotheses,
 * [1] scores, [2] selection, [3] motion hypotheses, [4] CheckRT, [5] the k-th cosine, [6] acceptance (with the gather of the candidate hypothesis' entries where the stages are not kept). Zeros without the variable and for
 * iba_debug_twoview_host. Same results. IBA_TWOVIEW_BUDGET: the bytes a chunk of pairs may take on the device in place of 1 GiB (same results). */
iba_status iba_debug_twoview_stage_ms(const iba_twoview_batch* r, float ms[7]);
/* debug: iba_pose_optimize as the host restatement of its rules (csrc/iba_pose_host.hpp over csrc/iba_pose_math.hpp), the whole call without a
 * device; the result is read with the iba_pose_* accessors. Byte for byte what the device gives (tests/test_gpu_pose.py). */
iba_status iba_debug_pose_host(const iba_pose_job* jobs, int32_t B, const iba_pose_options* opt, iba_pose_batch** out);
/* debug: iba_pose_eval on the host, the same outputs */
iba_status iba_debug_pose_eval_host(const iba_pose_job* jobs, int32_t B, const uint8_t* const* active, int32_t robust, double* H, double* b, double* chi2_robust,
                                    double* const* chi2_edges);
/* debug: rule P6's three coefficients at s = theta^2 <= pi^2 (host only): out = sin(th)/th, (1 - cos(th))/th^2, (th - sin(th))/th^3 */
iba_status iba_debug_pose_series(double s, double out[3]);
/* debug: Exp(dx) T of rule P6 on the host; *big = 1 where theta > pi took libm */
iba_status iba_debug_pose_exp(const double dx[6], const double T[12], double Tn[12], int32_t* big);
/* debug: the steps of the call beyond theta = pi (rule P6), the chunks it ran as, and the kernel time in ms from HIP events summed over the chunks;
 * 0 for NULL */
int32_t iba_debug_pose_big_steps(const iba_pose_batch* r);
int32_t iba_debug_pose_chunks(const iba_pose_batch* r);
float   iba_debug_pose_kernel_ms(const iba_pose_batch* r);

/* debug: iba_bundle_optimize as the host restatement of its rules (csrc/iba_bundle_host.hpp over csrc/iba_bundle_math.hpp, the text the kernels
 * compile), the whole call without a device; the result is read with the iba_bundle_* accessors. Byte for byte what the device gives
 * (tests/test_gpu_bundle.py). */
iba_status iba_debug_bundle_host(const iba_bundle_job* jobs, int32_t B, const iba_bundle_options* opt, iba_bundle_batch** out);
/* debug: iba_bundle_eval on the host, the same outputs */
iba_status iba_debug_bundle_eval_host(const iba_bundle_job* jobs, int32_t B, const uint8_t* const* active, int32_t robust, double lambda, iba_bundle_eval_out* outs);
/* debug: the steps of the call beyond theta = pi (rule P6), the chunks it ran as, and the time in ms from HIP events around the launch chains of
 * the chunks (the host's one-word reads between the steps included), summed over the chunks; 0 for NULL */
int32_t iba_debug_bundle_big_steps(const iba_bundle_batch* r);
int32_t iba_debug_bundle_chunks(const iba_bundle_batch* r);
float   iba_debug_bundle_kernel_ms(const iba_bundle_batch* r);

/* debug: iba_map_match as the host restatement of its rules (csrc/iba_map_match_host.hpp over csrc/iba_map_match_math.hpp, the text the kernels
 * compile), the whole call without a device; the same checks, the same result object and accessors. Byte for byte what the device gives
 * (tests/test_gpu_map_match.py). */
iba_status iba_debug_map_match_host(const iba_orb_frame* frames, int32_t F, const iba_map_points* points, const iba_map_match_job* jobs, int32_t J, const iba_map_match_options* opt,
                                    iba_map_matches** out);
/* debug: the chunks the jobs of the call behind m were cut into (IBA_MAP_MATCH_BUDGET: bytes a chunk's candidate lists may take in place of
 * IBA_MAP_MATCH_BUDGET_BYTES and the free-memory rule, read at every call under IBA_DEBUG_ENV=1; same results); 0 for iba_debug_map_match_host and
 * for NULL */
int32_t iba_debug_map_match_chunks(const iba_map_matches* m);
/* debug: with IBA_MAP_MATCH_TIMING set at the call (under IBA_DEBUG_ENV=1), times in ms from HIP events, summed over the chunks: [0] frustum,
 * [1] grid (cell, scan, fill) + list count, [2] scan + list write with the distances, [3] resolve. Zeros without the variable. Same results. */
iba_status iba_debug_map_match_stage_ms(const iba_map_matches* m, float ms[4]);

/* debug: iba_triangulate as the host restatement of its rules (csrc/iba_triangulate_host.hpp over csrc/iba_triangulate_math.hpp, the text the
 * kernels compile), the whole call without a device, neighbour after neighbour as the reference runs; the same checks, the same result object and
 * accessors. Byte for byte what the device gives (tests/test_gpu_triangulate.py). */
iba_status iba_debug_triangulate_host(const iba_orb_frame* frames, int32_t F, const iba_triangulate_keyframe* keyframes, int32_t K, const iba_triangulate_job* jobs, int32_t J,
                                      const iba_triangulate_options* opt, iba_triangulation** out);
/* debug: the chunks the jobs of the call behind t were cut into (IBA_TRIANGULATE_BUDGET: bytes a chunk's slots may take in place of
 * IBA_TRIANGULATE_BUDGET_BYTES and the free-memory rule, read at every call under IBA_DEBUG_ENV=1; same results); 0 for iba_debug_triangulate_host
 * and for NULL */
int32_t iba_debug_triangulate_chunks(const iba_triangulation* t);
/* debug: with IBA_TRIANGULATE_TIMING set at the call (under IBA_DEBUG_ENV=1), times in ms from HIP events, summed over the chunks: [0] prologue +
 * segments, [1] pick, [2] compaction + triangulation, [3] resolve, counts, scan and gather. Zeros without the variable. Same results. */
iba_status iba_debug_triangulate_stage_ms(const iba_triangulation* t, float ms[4]);

/* debug: iba_fuse as the host restatement of its rules (csrc/iba_fuse_host.hpp over csrc/iba_fuse_math.hpp, the text the kernels compile), the
 * whole call without a device; the same checks, the same result object and accessors, iba_fuse_apply included. Byte for byte what the device
 * gives (tests/test_gpu_fuse.py). */
iba_status iba_debug_fuse_host(const iba_orb_frame* frames, int32_t F, const iba_map_points* points, const iba_fuse_job* jobs, int32_t J, const iba_fuse_options* opt, iba_fusion** out);
/* debug: the chunks the jobs of the call behind f were cut into (IBA_FUSE_BUDGET: bytes a chunk's candidate lists may take in place of
 * IBA_FUSE_BUDGET_BYTES and the free-memory rule, read at every call under IBA_DEBUG_ENV=1; same results); 0 for iba_debug_fuse_host and for NULL */
int32_t iba_debug_fuse_chunks(const iba_fusion* f);
/* debug: with IBA_FUSE_TIMING set at the call (under IBA_DEBUG_ENV=1), times in ms from HIP events, summed over the chunks: [0] frustum, [1] grid
 * (cell, scan, fill) + list count, [2] scan + list write with the distances, [3] pick. Zeros without the variable. Same results. */
iba_status iba_debug_fuse_stage_ms(const iba_fusion* f, float ms[4]);

/* debug: iba_refresh as the host restatement of its rules (csrc/iba_refresh_host.hpp over csrc/iba_refresh_math.hpp, the text the kernels compile;
 * S3's rank form through a histogram of every row), the whole call without a device; the same checks, the same result object and accessors,
 * iba_refresh_store included; counts.path is zero. Byte for byte what the device gives (tests/test_gpu_refresh.py). */
iba_status iba_debug_refresh_host(const iba_orb_frame* frames, int32_t F, const iba_refresh_keyframe* keyframes, int32_t K, const iba_map_points* points, const uint8_t* point_bad,
                                  const int32_t* ref_keyframe, const int32_t* obs_off, const int32_t* obs_keyframe, const int32_t* obs_keypoint, const int32_t* list, int32_t n,
                                  const iba_refresh_options* opt, iba_refreshed** out);
/* debug: with IBA_REFRESH_TIMING set at the call (under IBA_DEBUG_ENV=1), times in ms from HIP events: [0] the narrow, [1] the wave, [2] the block
 * launch. Zeros without the variable. Same results. */
iba_status iba_debug_refresh_stage_ms(const iba_refreshed* r, float ms[3]);

/* debug: iba_sim3_solve as the host restatement of its rules (csrc/iba_sim3_host.hpp over csrc/iba_sim3_math.hpp, the text the kernels compile),
 * the whole call without a device; the same checks, the same result object and accessors. Byte for byte what the device gives
 * (tests/test_gpu_sim3.py). */
iba_status iba_debug_sim3_host(const iba_map_points* points, const iba_sim3_job* jobs, int32_t J, const iba_sim3_options* opt, iba_sim3_batch** out);
/* debug: the chunks the call was cut into (0 from the host restatement) */
int32_t    iba_debug_sim3_chunks(const iba_sim3_batch* r);
/* debug: with IBA_SIM3_TIMING set at the call (under IBA_DEBUG_ENV=1), times in ms from HIP events, summed over the chunks: [0] preparation,
 * [1] hypotheses, [2] the count kernel, [3] selection, [4] flags. Zeros without the variable. Same results. */
iba_status iba_debug_sim3_stage_ms(const iba_sim3_batch* r, float ms[5]);

#ifdef __cplusplus
}
#endif
#endif /* IBA_MI355X_DEBUG_H */
