// Host side of the Scan Context entry points (include/iba_mi355x.h; included at the end of iba_capi.hip, whose handle and HIP_TRY it uses).
// iba_sc_describe: one launch chain on the handle's stream (memset of the bins, bins kernel, finalise kernel) and one synchronise; down go the node ->
// frame list and the slice list (4 + 8 B per entry), nothing comes up. The database owns its device arrays and a stream of its own, so it outlives the
// handle. iba_sc_detect: queries down (16 B each), search -> distances -> pick on the database's stream, one synchronise, the results up (240 B each).
// iba_sc_replay_plan and iba_default_sc_options touch no device.
struct iba_sc_db {
    int device = 0;
    int32_t n = 0, R = 0, S = 0;
    double max_radius = 0.0, lidar_height = 0.0;
    hipStream_t stream = nullptr;
    DevBuf<double> desc, ring_key, sector_key, col_norm;
    DevBuf<float> ring_key_f;
    DevBuf<uint32_t> skipped;
    // work buffers of the calls on this database, grown on demand
    DevBuf<iba_sc_query> d_q; DevBuf<int32_t> d_cand, d_pairs, d_shift; DevBuf<double> d_dist; DevBuf<iba_sc_result> d_res;
    std::string err;
};

namespace {

constexpr int kScMaxNodes = 1 << 20;
constexpr int kScMaxQueries = 65536;
constexpr int kScMaxPairs = 1 << 20;

iba_status sc_fail(iba_sc_db* db, iba_status s, const std::string& msg) { if (db) db->err = msg; else g_create_error = msg; return s; }

// "" when the options are inside the supported range
std::string sc_check_options(const iba_sc_options* o) {
    if (!o) return "the options are NULL";
    if (o->struct_size != (int32_t)sizeof(iba_sc_options)) return "iba_sc_options.struct_size does not match this library";
    if (o->num_ring < 1 || o->num_ring > IBA_SC_MAX_RING) return "num_ring must be in [1, 64]";
    if (o->num_sector < 1 || o->num_sector > IBA_SC_MAX_SECTOR) return "num_sector must be in [1, 256]";
    if (o->num_candidates < 1 || o->num_candidates > IBA_SC_MAX_CANDIDATES) return "num_candidates must be in [1, 16]";
    if (!(o->max_radius > 0.0) || !std::isfinite(o->max_radius)) return "max_radius must be positive and finite";
    if (!std::isfinite(o->lidar_height)) return "lidar_height is not finite";
    if (!(o->search_ratio >= 0.0) || !std::isfinite(o->search_ratio)) return "search_ratio must be finite and not negative";
    if (!std::isfinite(o->dist_thres)) return "dist_thres is not finite";
    if (o->num_exclude_recent < 0) return "num_exclude_recent must not be negative";
    if (o->tree_period < 1) return "tree_period must be at least 1";
    return "";
}

ScShape sc_shape(const iba_sc_options& o) {
    ScShape s{};
    s.R = o.num_ring; s.S = o.num_sector; s.k = o.num_candidates;
    const double rad = std::floor(0.5 * o.search_ratio * (double)o.num_sector + 0.5);   // round() of a non-negative value
    s.radius = (int)std::min(rad, (double)o.num_sector);
    s.max_radius = o.max_radius; s.lidar_height = o.lidar_height; s.dist_thres = o.dist_thres;
    return s;
}

iba_status sc_check_db(iba_sc_db* db, const iba_sc_options* opt, const char* who) {
    const std::string bad = sc_check_options(opt);
    if (!bad.empty()) return sc_fail(db, IBA_ERR_INVALID_ARG, std::string(who) + ": " + bad);
    if (opt->num_ring != db->R || opt->num_sector != db->S)
        return sc_fail(db, IBA_ERR_INVALID_ARG, std::string(who) + ": num_ring x num_sector of the options (" + std::to_string(opt->num_ring) + " x " + std::to_string(opt->num_sector) + ") differ from the database's (" +
                                                    std::to_string(db->R) + " x " + std::to_string(db->S) + ")");
    return IBA_OK;
}

// the distance launch of both callers: pairs (iba_sc_distance) or queries + candidates (iba_sc_detect)
iba_status sc_launch_distance(iba_sc_db* db, const ScShape& sh, const int32_t* d_pairs, const iba_sc_query* d_q, const int32_t* d_cand, unsigned n_blocks, double* d_dist, int32_t* d_shift) {
    const bool staged = sc_distance_lds(sh.R, sh.S, true) <= 65536;
    const size_t lds = sc_distance_lds(sh.R, sh.S, staged);
    if (staged) hipLaunchKernelGGL(iba_sc_distance_kernel<true>, dim3(n_blocks), dim3(64), lds, db->stream, db->desc.p, db->sector_key.p, db->col_norm.p, d_pairs, d_q, d_cand, sh, d_dist, d_shift);
    else hipLaunchKernelGGL(iba_sc_distance_kernel<false>, dim3(n_blocks), dim3(64), lds, db->stream, db->desc.p, db->sector_key.p, db->col_norm.p, d_pairs, d_q, d_cand, sh, d_dist, d_shift);
    HIP_TRY(db, hipGetLastError());
    return IBA_OK;
}

}  // namespace

iba_status iba_default_sc_options(iba_sc_options* o) {
    if (!o) return sc_fail(nullptr, IBA_ERR_INVALID_ARG, "iba_default_sc_options: the options are NULL");
    std::memset(o, 0, sizeof(*o));
    o->struct_size = (int32_t)sizeof(*o);
    o->num_ring = 20; o->num_sector = 60; o->num_exclude_recent = 30; o->num_candidates = 3; o->tree_period = 30;
    o->max_radius = 80.0; o->lidar_height = 0.0; o->search_ratio = 0.1; o->dist_thres = 0.2;
    return IBA_OK;
}

const char* iba_sc_last_error(const iba_sc_db* db) { return db ? db->err.c_str() : g_create_error.c_str(); }
int32_t iba_sc_db_size(const iba_sc_db* db) { return db ? db->n : 0; }
void iba_sc_db_free(iba_sc_db* db) {
    if (!db) return;
    (void)hipSetDevice(db->device);
    if (db->stream) (void)hipStreamDestroy(db->stream);
    delete db;
}

iba_status iba_sc_replay_plan(const int32_t* sizes_at_call, int32_t n, const iba_sc_options* opt, int32_t* db_end) {
    const std::string who = "iba_sc_replay_plan: ";
    if (!sizes_at_call || !db_end) return sc_fail(nullptr, IBA_ERR_INVALID_ARG, who + "sizes_at_call / db_end are NULL");
    const std::string bad = sc_check_options(opt);
    if (!bad.empty()) return sc_fail(nullptr, IBA_ERR_INVALID_ARG, who + bad);
    if (n < 1) return sc_fail(nullptr, IBA_ERR_INVALID_ARG, who + "n must be at least 1");
    for (int32_t i = 0; i < n; ++i)
        if (sizes_at_call[i] < 1) return sc_fail(nullptr, IBA_ERR_INVALID_ARG, who + "call " + std::to_string(i) + " holds " + std::to_string(sizes_at_call[i]) + " descriptors: a call needs at least its own");
    int64_t counter = 0;
    int32_t cur = 0;
    for (int32_t i = 0; i < n; ++i) {
        const int32_t size = sizes_at_call[i];
        if (size < opt->num_exclude_recent + 1) { db_end[i] = 0; continue; }   // the early return: the counter does not advance
        if (counter % opt->tree_period == 0) cur = size - opt->num_exclude_recent;
        ++counter;
        db_end[i] = cur;
    }
    return IBA_OK;
}

iba_status iba_sc_describe(iba_handle* h, const int32_t* frames, int32_t n, const iba_sc_options* opt, iba_sc_db** out) {
    const std::string who = "iba_sc_describe: ";
    if (!h) return sc_fail(nullptr, IBA_ERR_INVALID_ARG, who + "the handle is NULL");
    if (!out) return fail(h, IBA_ERR_INVALID_ARG, who + "the result pointer is NULL");
    *out = nullptr;
    if (!frames) return fail(h, IBA_ERR_INVALID_ARG, who + "frames is NULL");
    const std::string bad = sc_check_options(opt);
    if (!bad.empty()) return fail(h, IBA_ERR_INVALID_ARG, who + bad);
    if (n < 1 || n > kScMaxNodes) return fail(h, IBA_ERR_INVALID_ARG, who + "n must be in [1, 2^20]");
    std::vector<ScBlock> blocks;
    for (int32_t i = 0; i < n; ++i) {
        if (frames[i] < 0 || frames[i] >= h->n_frames)
            return fail(h, IBA_ERR_INVALID_ARG, who + "node " + std::to_string(i) + " names frame " + std::to_string(frames[i]) + " outside the handle's " + std::to_string(h->n_frames) + " local frames");
        const uint32_t P = h->h_frames[(size_t)frames[i]].P;
        for (uint64_t b = 0; b < P; b += (uint64_t)kScSlice) blocks.push_back(ScBlock{i, (uint32_t)b});
        if (blocks.size() > 0x7FFFFFFFull) return fail(h, IBA_ERR_UNSUPPORTED, who + "the nodes of one call hold more than 2^31 slices of 4096 points (split the call)");
    }
    const ScShape sh = sc_shape(*opt);
    const size_t nb = (size_t)sh.R * (size_t)sh.S;

    HIP_TRY(h, hipSetDevice(h->device));
    std::unique_ptr<iba_sc_db, decltype(&iba_sc_db_free)> db(new iba_sc_db, iba_sc_db_free);   // (freed on every error path below)
    db->device = h->device; db->n = n; db->R = sh.R; db->S = sh.S; db->max_radius = sh.max_radius; db->lidar_height = sh.lidar_height;
    HIP_TRY(h, hipStreamCreateWithFlags(&db->stream, hipStreamNonBlocking));
    HIP_TRY(h, db->desc.alloc((size_t)n * nb)); HIP_TRY(h, db->ring_key.alloc((size_t)n * sh.R)); HIP_TRY(h, db->ring_key_f.alloc((size_t)n * sh.R));
    HIP_TRY(h, db->sector_key.alloc((size_t)n * sh.S)); HIP_TRY(h, db->col_norm.alloc((size_t)n * sh.S)); HIP_TRY(h, db->skipped.alloc((size_t)n));
    DevBuf<uint32_t> d_bins; DevBuf<int32_t> d_frames; DevBuf<ScBlock> d_blocks;
    HIP_TRY(h, d_bins.alloc((size_t)n * nb)); HIP_TRY(h, d_frames.alloc((size_t)n)); HIP_TRY(h, d_blocks.alloc(blocks.size()));
    const hipStream_t st = h->stream;
    HIP_TRY(h, hipMemcpyAsync(d_frames.p, frames, sizeof(int32_t) * (size_t)n, hipMemcpyHostToDevice, st));
    if (!blocks.empty()) HIP_TRY(h, hipMemcpyAsync(d_blocks.p, blocks.data(), sizeof(ScBlock) * blocks.size(), hipMemcpyHostToDevice, st));
    HIP_TRY(h, hipMemsetAsync(d_bins.p, 0, sizeof(uint32_t) * (size_t)n * nb, st));
    HIP_TRY(h, hipMemsetAsync(db->skipped.p, 0, sizeof(uint32_t) * (size_t)n, st));
    if (!blocks.empty()) {   // (every node an empty scan: all bins stay empty)
        HIP_TRY(h, hipFuncSetAttribute((const void*)iba_sc_bins_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, 65536));
        hipLaunchKernelGGL(iba_sc_bins_kernel, dim3((unsigned)blocks.size()), dim3(kScThreads), nb * sizeof(uint32_t), st, h->frames.p, h->pts4.p, d_frames.p, d_blocks.p, sh, d_bins.p, db->skipped.p);
        HIP_TRY(h, hipGetLastError());
    }
    hipLaunchKernelGGL(iba_sc_finalize_kernel, dim3((unsigned)n), dim3(64), 0, st, d_bins.p, sh, db->desc.p, db->ring_key.p, db->ring_key_f.p, db->sector_key.p, db->col_norm.p);
    HIP_TRY(h, hipGetLastError());
    HIP_TRY(h, hipStreamSynchronize(st));
    *out = db.release();
    return IBA_OK;
}

iba_status iba_sc_db_read(iba_sc_db* db, int32_t first, int32_t count, double* desc, double* ring_key, float* ring_key_f, double* sector_key, int64_t* n_skipped) {
    if (!db) return sc_fail(nullptr, IBA_ERR_INVALID_ARG, "iba_sc_db_read: the database is NULL");
    if (first < 0 || count < 0 || (int64_t)first + count > db->n)
        return sc_fail(db, IBA_ERR_INVALID_ARG, "iba_sc_db_read: nodes [" + std::to_string(first) + ", " + std::to_string((int64_t)first + count) + ") are outside the database's " + std::to_string(db->n));
    if (count == 0) return IBA_OK;
    HIP_TRY(db, hipSetDevice(db->device));
    const size_t nb = (size_t)db->R * (size_t)db->S, f = (size_t)first, c = (size_t)count;
    std::vector<uint32_t> sk;
    if (desc) HIP_TRY(db, hipMemcpyAsync(desc, db->desc.p + f * nb, sizeof(double) * c * nb, hipMemcpyDeviceToHost, db->stream));
    if (ring_key) HIP_TRY(db, hipMemcpyAsync(ring_key, db->ring_key.p + f * db->R, sizeof(double) * c * db->R, hipMemcpyDeviceToHost, db->stream));
    if (ring_key_f) HIP_TRY(db, hipMemcpyAsync(ring_key_f, db->ring_key_f.p + f * db->R, sizeof(float) * c * db->R, hipMemcpyDeviceToHost, db->stream));
    if (sector_key) HIP_TRY(db, hipMemcpyAsync(sector_key, db->sector_key.p + f * db->S, sizeof(double) * c * db->S, hipMemcpyDeviceToHost, db->stream));
    if (n_skipped) { sk.resize(c); HIP_TRY(db, hipMemcpyAsync(sk.data(), db->skipped.p + f, sizeof(uint32_t) * c, hipMemcpyDeviceToHost, db->stream)); }
    HIP_TRY(db, hipStreamSynchronize(db->stream));
    if (n_skipped) for (size_t i = 0; i < c; ++i) n_skipped[i] = (int64_t)sk[i];
    return IBA_OK;
}

iba_status iba_sc_distance(iba_sc_db* db, const int32_t* pairs, int32_t P, const iba_sc_options* opt, double* dist, int32_t* shift) {
    const std::string who = "iba_sc_distance: ";
    if (!db) return sc_fail(nullptr, IBA_ERR_INVALID_ARG, who + "the database is NULL");
    if (!pairs || !dist || !shift) return sc_fail(db, IBA_ERR_INVALID_ARG, who + "pairs / dist / shift are NULL");
    if (const iba_status s = sc_check_db(db, opt, "iba_sc_distance")) return s;
    if (P < 1 || P > kScMaxPairs) return sc_fail(db, IBA_ERR_INVALID_ARG, who + "P must be in [1, 2^20]");
    for (int32_t p = 0; p < 2 * P; ++p)
        if (pairs[p] < 0 || pairs[p] >= db->n)
            return sc_fail(db, IBA_ERR_INVALID_ARG, who + "pair " + std::to_string(p / 2) + " names node " + std::to_string(pairs[p]) + " outside the database's " + std::to_string(db->n) + " nodes");
    const ScShape sh = sc_shape(*opt);
    HIP_TRY(db, hipSetDevice(db->device));
    HIP_TRY(db, db->d_pairs.grow(2 * (size_t)P)); HIP_TRY(db, db->d_dist.grow((size_t)P)); HIP_TRY(db, db->d_shift.grow((size_t)P));
    HIP_TRY(db, hipMemcpyAsync(db->d_pairs.p, pairs, sizeof(int32_t) * 2 * (size_t)P, hipMemcpyHostToDevice, db->stream));
    if (const iba_status s = sc_launch_distance(db, sh, db->d_pairs.p, nullptr, nullptr, (unsigned)P, db->d_dist.p, db->d_shift.p)) return s;
    HIP_TRY(db, hipMemcpyAsync(dist, db->d_dist.p, sizeof(double) * (size_t)P, hipMemcpyDeviceToHost, db->stream));
    HIP_TRY(db, hipMemcpyAsync(shift, db->d_shift.p, sizeof(int32_t) * (size_t)P, hipMemcpyDeviceToHost, db->stream));
    HIP_TRY(db, hipStreamSynchronize(db->stream));
    return IBA_OK;
}

iba_status iba_sc_detect(iba_sc_db* db, const iba_sc_query* queries, int32_t Q, const iba_sc_options* opt, iba_sc_result* out) {
    const std::string who = "iba_sc_detect: ";
    if (!db) return sc_fail(nullptr, IBA_ERR_INVALID_ARG, who + "the database is NULL");
    if (!queries || !out) return sc_fail(db, IBA_ERR_INVALID_ARG, who + "queries / out are NULL");
    if (const iba_status s = sc_check_db(db, opt, "iba_sc_detect")) return s;
    if (Q < 1 || Q > kScMaxQueries) return sc_fail(db, IBA_ERR_INVALID_ARG, who + "Q must be in [1, 65536]");
    for (int32_t q = 0; q < Q; ++q) {
        const std::string at = who + "query " + std::to_string(q) + ": ";
        if (queries[q].struct_size != (int32_t)sizeof(iba_sc_query)) return sc_fail(db, IBA_ERR_INVALID_ARG, at + "iba_sc_query.struct_size does not match this library");
        if (queries[q].node < 0 || queries[q].node >= db->n) return sc_fail(db, IBA_ERR_INVALID_ARG, at + "node " + std::to_string(queries[q].node) + " is outside the database's " + std::to_string(db->n) + " nodes");
        if (queries[q].db_end < 0 || queries[q].db_end > db->n) return sc_fail(db, IBA_ERR_INVALID_ARG, at + "db_end " + std::to_string(queries[q].db_end) + " is beyond the database's " + std::to_string(db->n) + " nodes");
    }
    const ScShape sh = sc_shape(*opt);
    const size_t QK = (size_t)Q * (size_t)sh.k;
    HIP_TRY(db, hipSetDevice(db->device));
    HIP_TRY(db, db->d_q.grow((size_t)Q)); HIP_TRY(db, db->d_cand.grow(QK)); HIP_TRY(db, db->d_dist.grow(QK)); HIP_TRY(db, db->d_shift.grow(QK));
    HIP_TRY(db, db->d_res.grow((size_t)Q));
    HIP_TRY(db, hipMemcpyAsync(db->d_q.p, queries, sizeof(iba_sc_query) * (size_t)Q, hipMemcpyHostToDevice, db->stream));
    hipLaunchKernelGGL(iba_sc_knn_kernel, dim3((unsigned)Q), dim3(64), 0, db->stream, db->ring_key_f.p, db->d_q.p, sh, db->d_cand.p);
    HIP_TRY(db, hipGetLastError());
    if (const iba_status s = sc_launch_distance(db, sh, nullptr, db->d_q.p, db->d_cand.p, (unsigned)QK, db->d_dist.p, db->d_shift.p)) return s;
    hipLaunchKernelGGL(iba_sc_pick_kernel, dim3((unsigned)((Q + 255) / 256)), dim3(256), 0, db->stream, db->d_q.p, db->d_cand.p, db->d_dist.p, db->d_shift.p, sh, (int)Q, db->d_res.p);
    HIP_TRY(db, hipGetLastError());
    HIP_TRY(db, hipMemcpyAsync(out, db->d_res.p, sizeof(iba_sc_result) * (size_t)Q, hipMemcpyDeviceToHost, db->stream));
    HIP_TRY(db, hipStreamSynchronize(db->stream));
    return IBA_OK;
}
