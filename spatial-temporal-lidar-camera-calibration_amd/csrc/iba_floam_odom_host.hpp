// Host side of iba_floam_odom_run (include/iba_mi355x.h; included at the end of iba_capi.hip, after the hosts whose chains it drives). One call =
//   1  ONE extract chain over every scan of every track, its two gathered clouds left on the device (floam_extract_impl, iba_floam_host.hpp);
//   2  the raw feature clouds made the frames of a handle F (iba_floam_odom_move_kernel widens them, scan_handle_from_device indexes them) and ONE
//      lattice chain over its 2 n frames: the down-sampled clouds of every scan, left in F's voxel buffer;
//   3  step 0 of every track: the raw features moved by T0 (the move kernel again) are the first map;
//   4  per step k >= 1, for all tracks still running together: the four clouds of every track (down-sampled scan k out of F, the map of step
//      k - 1) copied device-to-device into one staging buffer, a small handle H_k built from it on the device, iba_floam_map_register on H_k from
//      the predicted poses, then ONE lattice chain on H_k (members: old map, identity; scan cloud, T[k]; crop t[k] +- crop_half) whose result —
//      the new maps — stays in H_k's voxel buffer until H_k+1 is staged from it.
// What a step allocates: the staging buffer (24 B per point of the four clouds), H_k (a scans-only handle: its leaf-ordered arrays, kd nodes,
// boxes and plane memo, the index build's scratch of the size of the clouds for the time of the build, H_k's pass and voxel work buffers as
// they grow) and, with keep_maps or on a track's last step, a copy of the track's new map (24 B per point). H_k-1 is released once H_k exists.
// Between the upload of the track descriptors and the download of the results only the small per-step blocks cross PCIe (bounds, counts,
// frame boxes, LM moments, ring sizes); the maps and down-sampled clouds the accessors expose come down once, at the end.

struct iba_floam_odom {
    struct Track {
        std::vector<iba_floam_odom_step> steps;
        std::vector<std::vector<float>> src[2];   // [kind][k]: the down-sampled clouds
        std::vector<std::vector<float>> map[2];   // [kind][k]: the map after step k (kept steps only)
        std::vector<char> has_map;                // [k]
    };
    std::vector<Track> tracks;
};

namespace {

constexpr int kOdomMaxTracks = 256;
constexpr int kOdomMaxScans = 1 << 16;          // of one track
constexpr int kOdomMaxCallScans = kVoxMaxSubs / 2;   // of one call: the down-sampling chain takes two sub-maps per scan

struct OdomHandle {   // a handle the call created and releases
    iba_handle* p = nullptr;
    OdomHandle() = default;
    OdomHandle(const OdomHandle&) = delete;
    OdomHandle& operator=(const OdomHandle&) = delete;
    ~OdomHandle() { reset(nullptr); }
    void reset(iba_handle* q) { if (p) iba_destroy(p); p = q; }
};

struct OdomKept { int b, k; DevBuf<double> xyz; size_t n[2]; };   // a map that the result exposes: edge cloud, then surf cloud

void odom_inverse(const double* T, double* M) {   // [R^T, -R^T t]
    for (int r = 0; r < 3; ++r) {
        for (int c = 0; c < 3; ++c) M[4 * r + c] = T[4 * c + r];
        M[4 * r + 3] = -((T[r] * T[3] + T[4 + r] * T[7]) + T[8 + r] * T[11]);
    }
    M[12] = 0.0; M[13] = 0.0; M[14] = 0.0; M[15] = 1.0;
}

void odom_narrow(const double* src, size_t n_pts, std::vector<float>& dst) {
    dst.resize(3 * n_pts);
    for (size_t i = 0; i < 3 * n_pts; ++i) dst[i] = (float)src[i];
}

iba_status odom_move(iba_handle* h, const std::vector<OdomSegment>& segs, const FloamDevClouds& dev, double* out, DevBuf<OdomSegment>& d_segs) {
    uint32_t maxn = 0;
    for (const OdomSegment& s : segs) maxn = std::max(maxn, s.n);
    if (segs.empty() || maxn == 0) return IBA_OK;
    HIP_TRY(h, d_segs.grow(segs.size()));
    HIP_TRY(h, hipMemcpyAsync(d_segs.p, segs.data(), sizeof(OdomSegment) * segs.size(), hipMemcpyHostToDevice, h->stream));
    hipLaunchKernelGGL(iba_floam_odom_move_kernel, dim3((maxn + (uint32_t)kVoxThreads - 1u) / (uint32_t)kVoxThreads, (unsigned)segs.size()), dim3(kVoxThreads), 0, h->stream, d_segs.p, dev.exyz.p, dev.sxyz.p, out);
    HIP_TRY(h, hipGetLastError());
    HIP_TRY(h, hipStreamSynchronize(h->stream));   // (segs is the caller's pageable memory)
    return IBA_OK;
}

void odom_lattice_desc(iba_lattice_desc& d, int32_t n_members, const int32_t* frames, const double* poses12, double leaf) {
    std::memset(&d, 0, sizeof(d));
    d.struct_size = (int32_t)sizeof(d); d.n_members = n_members; d.frames = frames; d.poses12 = poses12; d.leaf = leaf;
}

}  // namespace

iba_status iba_default_floam_odom_options(iba_floam_odom_options* o) {
    if (!o) return fail(nullptr, IBA_ERR_INVALID_ARG, "iba_default_floam_odom_options: the options are NULL");
    std::memset(o, 0, sizeof(*o));
    o->struct_size = (int32_t)sizeof(*o);
    o->init_passes = 12; o->keep_maps = 0; o->map_resolution = 0.4; o->crop_half = 100.0;
    iba_default_floam_options(&o->extract);
    iba_default_floam_map_options(&o->map);
    return IBA_OK;
}

iba_status iba_floam_odom_run(iba_handle* h, const iba_floam_track* tracks, int32_t B, const iba_floam_odom_options* opt, iba_floam_odom** out) {
    const std::string who = "iba_floam_odom_run: ";
    if (!h) return fail(nullptr, IBA_ERR_INVALID_ARG, who + "the handle is NULL");
    if (!out) return fail(h, IBA_ERR_INVALID_ARG, who + "the result pointer is NULL");
    *out = nullptr;
    if (!tracks) return fail(h, IBA_ERR_INVALID_ARG, who + "the tracks are NULL");
    if (!opt) return fail(h, IBA_ERR_INVALID_ARG, who + "the options are NULL (iba_default_floam_odom_options fills them)");
    if (opt->struct_size != (int32_t)sizeof(iba_floam_odom_options)) return fail(h, IBA_ERR_INVALID_ARG, who + "iba_floam_odom_options.struct_size does not match this library");
    if (B < 1 || B > kOdomMaxTracks) return fail(h, IBA_ERR_INVALID_ARG, who + "B must be in [1, 256]");
    if (!(opt->map_resolution > 0.0) || !std::isfinite(opt->map_resolution)) return fail(h, IBA_ERR_INVALID_ARG, who + "map_resolution must be positive and finite");
    if (!(opt->crop_half > 0.0) || !std::isfinite(opt->crop_half)) return fail(h, IBA_ERR_INVALID_ARG, who + "crop_half must be positive and finite");
    if (opt->init_passes < 0) return fail(h, IBA_ERR_INVALID_ARG, who + "init_passes must not be negative");
    {
        const std::string bad = floam_check_options(&opt->extract);
        if (!bad.empty()) return fail(h, IBA_ERR_INVALID_ARG, who + "extract: " + bad);
        const std::string badm = fmap_options_error(&opt->map, "iba_floam_odom_run");
        if (!badm.empty()) return fail(h, IBA_ERR_INVALID_ARG, who + "map: " + badm);
    }
    std::vector<int32_t> scan0((size_t)B + 1, 0), frames_all;
    int max_scans = 0;
    for (int b = 0; b < B; ++b) {
        const iba_floam_track& t = tracks[b];
        const std::string at = who + "track " + std::to_string(b) + ": ";
        if (t.n_scans < 1 || t.n_scans > kOdomMaxScans) return fail(h, IBA_ERR_INVALID_ARG, at + "n_scans must be in [1, 65536]");
        if (!t.frames) return fail(h, IBA_ERR_INVALID_ARG, at + "frames is NULL");
        for (int k = 0; k < t.n_scans; ++k)
            if (t.frames[k] < 0 || t.frames[k] >= h->n_frames)
                return fail(h, IBA_ERR_INVALID_ARG, at + "scan " + std::to_string(k) + " names frame " + std::to_string(t.frames[k]) + " outside the handle's " + std::to_string(h->n_frames) + " local frames");
        if (!icp_finite16(t.T0)) return fail(h, IBA_ERR_INVALID_ARG, at + "T0 is not finite");
        frames_all.insert(frames_all.end(), t.frames, t.frames + t.n_scans);
        scan0[(size_t)b + 1] = scan0[(size_t)b] + t.n_scans;
        max_scans = std::max(max_scans, (int)t.n_scans);
        if (scan0[(size_t)b + 1] > kOdomMaxCallScans) return fail(h, IBA_ERR_UNSUPPORTED, who + "the tracks of one call hold more than " + std::to_string(kOdomMaxCallScans) + " scans (split the batch)");
    }
    const int32_t n = scan0[(size_t)B];
    const double res[2] = {opt->map_resolution, 2.0 * opt->map_resolution};
    const double I12[12] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0};

    // ---- 1: the features of every scan, on the device ----
    FloamDevClouds dev;
    iba_floam_features* feat_raw = nullptr;
    if (const iba_status s = floam_extract_impl(h, frames_all.data(), n, &opt->extract, who, &dev, &feat_raw)) return s;
    const std::unique_ptr<iba_floam_features> feat(feat_raw);
    const int64_t NE = feat->efirst[(size_t)n], NS = feat->sfirst[(size_t)n];
    const int64_t* ffirst[2] = {feat->efirst.data(), feat->sfirst.data()};

    HIP_TRY(h, hipSetDevice(h->device));
    const hipStream_t st = h->stream;
    iba_params prm = h->params;
    prm.plane_cache = 1;   // (the memo is a record per point; plane_cache = 0 would reserve a record per point and batch slot)
    DevBuf<OdomSegment> d_segs;

    // ---- 2: the raw clouds as frames 2 i (edge), 2 i + 1 (surf) of F, and the down-sampling chain ----
    DevBuf<double> rawd;
    HIP_TRY(h, rawd.alloc(3 * (size_t)(NE + NS)));
    {
        std::vector<OdomSegment> segs;
        const int64_t tot[2] = {NE, NS};
        for (int kind = 0; kind < 2; ++kind)
            for (int64_t o = 0; o < tot[kind]; o += 0x40000000ll) {   // (a segment's length is a 32-bit value)
                OdomSegment sg;
                std::memset(&sg, 0, sizeof(sg));
                sg.src0 = (uint64_t)o; sg.dst0 = (uint64_t)((kind ? NE : 0) + o); sg.n = (uint32_t)std::min<int64_t>(tot[kind] - o, 0x40000000ll); sg.kind = kind; sg.move = 0;
                segs.push_back(sg);
            }
        if (const iba_status s = odom_move(h, segs, dev, rawd.p, d_segs)) return s;
    }
    OdomHandle F;
    {
        std::vector<int64_t> first(2 * (size_t)n), counts(2 * (size_t)n);
        for (int i = 0; i < n; ++i)
            for (int kind = 0; kind < 2; ++kind) {
                first[2 * (size_t)i + kind] = (kind ? NE : 0) + ffirst[kind][i];
                counts[2 * (size_t)i + kind] = ffirst[kind][i + 1] - ffirst[kind][i];
            }
        if ((uint64_t)(NE + NS) > kVoxMaxPoints) return fail(h, IBA_ERR_UNSUPPORTED, who + "the feature clouds of one call hold more than 2^32 - 256 points (split the batch)");
        iba_handle* f = nullptr;
        if (const iba_status s = scan_handle_from_device(h, rawd.p, first, &counts, 2 * n, &prm, who, "feature cloud", &f)) return s;
        F.reset(f);
    }
    std::unique_ptr<iba_submap_clouds> ds;
    {
        std::vector<int32_t> fr(2 * (size_t)n);
        std::vector<iba_lattice_desc> descs(2 * (size_t)n);
        for (int i = 0; i < 2 * n; ++i) { fr[(size_t)i] = i; odom_lattice_desc(descs[(size_t)i], 1, &fr[(size_t)i], I12, res[i & 1]); }
        iba_submap_clouds* c = nullptr;
        if (const iba_status s = vox_build(F.p, descs.data(), 2 * n, who, false, &c)) return fail(h, s, F.p->err);
        ds.reset(c);
    }
    const double* d_ds = F.p->vox.d_xyz.p;   // the down-sampled clouds: sub-map 2 i + kind owns ds->first[2 i + kind] .. of it

    // ---- the result, step 0 of every track ----
    std::unique_ptr<iba_floam_odom> R(new iba_floam_odom);
    R->tracks.resize((size_t)B);
    for (int b = 0; b < B; ++b) {
        iba_floam_odom::Track& t = R->tracks[(size_t)b];
        const size_t ns = (size_t)tracks[b].n_scans;
        t.steps.assign(ns, iba_floam_odom_step{});
        for (int kind = 0; kind < 2; ++kind) { t.src[kind].resize(ns); t.map[kind].resize(ns); }
        t.has_map.assign(ns, 0);
        for (size_t k = 0; k < ns; ++k) {
            const size_t i = (size_t)scan0[(size_t)b] + k;
            t.steps[k].n_src_edge = ds->first[2 * i + 1] - ds->first[2 * i];
            t.steps[k].n_src_surf = ds->first[2 * i + 2] - ds->first[2 * i + 1];
        }
    }
    std::vector<OdomKept> kept;
    const auto keep_map = [&](int b, int k, const double* base, const int64_t off[2], const int64_t cnt[2]) -> hipError_t {
        kept.emplace_back();
        OdomKept& m = kept.back();
        m.b = b; m.k = k; m.n[0] = (size_t)cnt[0]; m.n[1] = (size_t)cnt[1];
        hipError_t e = m.xyz.alloc(3 * (m.n[0] + m.n[1]));
        if (e == hipSuccess && m.n[0]) e = hipMemcpyAsync(m.xyz.p, base + 3 * off[0], sizeof(double) * 3 * m.n[0], hipMemcpyDeviceToDevice, st);
        if (e == hipSuccess && m.n[1]) e = hipMemcpyAsync(m.xyz.p + 3 * m.n[0], base + 3 * off[1], sizeof(double) * 3 * m.n[1], hipMemcpyDeviceToDevice, st);
        return e;
    };

    // ---- 3: the first maps: the raw features of scan 0 moved by T0 ----
    std::vector<int64_t> map_off(2 * (size_t)B, 0), map_cnt(2 * (size_t)B, 0);   // [track][kind] in the current map buffer
    DevBuf<double> map0;
    const double* d_map = nullptr;
    {
        std::vector<OdomSegment> segs;
        int64_t total = 0;
        for (int b = 0; b < B; ++b)
            for (int kind = 0; kind < 2; ++kind) {
                const int i = scan0[(size_t)b];
                OdomSegment sg;
                std::memset(&sg, 0, sizeof(sg));
                for (int r = 0; r < 12; ++r) sg.T[r] = tracks[b].T0[r];
                sg.src0 = (uint64_t)ffirst[kind][i]; sg.dst0 = (uint64_t)total; sg.n = (uint32_t)(ffirst[kind][i + 1] - ffirst[kind][i]); sg.kind = kind; sg.move = 1;
                map_off[2 * (size_t)b + kind] = total; map_cnt[2 * (size_t)b + kind] = (int64_t)sg.n;
                total += (int64_t)sg.n;
                segs.push_back(sg);
            }
        HIP_TRY(h, map0.alloc(3 * (size_t)total));
        if (const iba_status s = odom_move(h, segs, dev, map0.p, d_segs)) return s;
        d_map = map0.p;
        for (int b = 0; b < B; ++b) {
            iba_floam_odom_step& s0 = R->tracks[(size_t)b].steps[0];
            std::memcpy(s0.T_pred, tracks[b].T0, sizeof(s0.T_pred)); std::memcpy(s0.T, tracks[b].T0, sizeof(s0.T));
            s0.status = IBA_FLOAM_MAP_OK;
            s0.n_map_edge = map_cnt[2 * (size_t)b]; s0.n_map_surf = map_cnt[2 * (size_t)b + 1];
            if (opt->keep_maps || tracks[b].n_scans == 1) HIP_TRY(h, keep_map(b, 0, d_map, &map_off[2 * (size_t)b], &map_cnt[2 * (size_t)b]));
        }
    }

    // ---- 4: the steps, all running tracks together ----
    OdomHandle prev;   // H_k-1: its voxel buffer holds the current maps
    for (int k = 1; k < max_scans; ++k) {
        std::vector<int> act;
        for (int b = 0; b < B; ++b) if (tracks[b].n_scans > k) act.push_back(b);
        const int Ba = (int)act.size();
        // the four clouds of every running track: frames 4 a .. 4 a + 3 = scan edge, scan surf, map edge, map surf
        std::vector<int64_t> first(4 * (size_t)Ba), counts(4 * (size_t)Ba);
        int64_t total = 0;
        for (int a = 0; a < Ba; ++a) {
            const int b = act[(size_t)a];
            const size_t i = (size_t)scan0[(size_t)b] + (size_t)k;
            const int64_t c[4] = {ds->first[2 * i + 1] - ds->first[2 * i], ds->first[2 * i + 2] - ds->first[2 * i + 1], map_cnt[2 * (size_t)b], map_cnt[2 * (size_t)b + 1]};
            for (int j = 0; j < 4; ++j) { first[4 * (size_t)a + j] = total; counts[4 * (size_t)a + j] = c[j]; total += c[j]; }
        }
        if ((uint64_t)total > kVoxMaxPoints) return fail(h, IBA_ERR_UNSUPPORTED, who + "the clouds of one step hold more than 2^32 - 256 points (split the batch)");
        DevBuf<double> stage;
        HIP_TRY(h, stage.alloc(3 * (size_t)total));
        for (int a = 0; a < Ba; ++a) {
            const int b = act[(size_t)a];
            const size_t i = (size_t)scan0[(size_t)b] + (size_t)k;
            const double* from[4] = {d_ds ? d_ds + 3 * ds->first[2 * i] : nullptr, d_ds ? d_ds + 3 * ds->first[2 * i + 1] : nullptr, d_map ? d_map + 3 * map_off[2 * (size_t)b] : nullptr,
                                     d_map ? d_map + 3 * map_off[2 * (size_t)b + 1] : nullptr};
            for (int j = 0; j < 4; ++j)
                if (counts[4 * (size_t)a + j] > 0)
                    HIP_TRY(h, hipMemcpyAsync(stage.p + 3 * first[4 * (size_t)a + j], from[j], sizeof(double) * 3 * (size_t)counts[4 * (size_t)a + j], hipMemcpyDeviceToDevice, st));
        }
        OdomHandle H;
        {
            iba_handle* hk = nullptr;
            if (const iba_status s = scan_handle_from_device(h, stage.p, first, &counts, 4 * Ba, &prm, who, "cloud", &hk)) return s;   // (runs on st, behind the copies, and waits for it)
            H.reset(hk);
        }
        // the prediction and the solve
        std::vector<iba_floam_pair> pairs((size_t)Ba);
        for (int a = 0; a < Ba; ++a) {
            const int b = act[(size_t)a];
            const std::vector<iba_floam_odom_step>& sp = R->tracks[(size_t)b].steps;
            const double* T1 = sp[(size_t)k - 1].T;
            const double* T2 = k >= 2 ? sp[(size_t)k - 2].T : tracks[b].T0;
            double inv2[16], delta[16];
            odom_inverse(T2, inv2);
            iba::icp::mat4_mul(inv2, T1, delta);
            iba_floam_pair& p = pairs[(size_t)a];
            p.src_edge_frame = 4 * a; p.src_surf_frame = 4 * a + 1; p.map_edge_frame = 4 * a + 2; p.map_surf_frame = 4 * a + 3;
            iba::icp::mat4_mul(T1, delta, p.T);
            p.T[12] = 0.0; p.T[13] = 0.0; p.T[14] = 0.0; p.T[15] = 1.0;
            if (!icp_finite16(p.T)) return fail(h, IBA_ERR_UNSUPPORTED, who + "track " + std::to_string(b) + ": the predicted pose of step " + std::to_string(k) + " is not finite");
        }
        iba_floam_map_options mopt = opt->map;
        mopt.outer_passes = std::max(opt->map.outer_passes, opt->init_passes - k);
        std::vector<iba_floam_map_result> sol((size_t)Ba);
        if (const iba_status s = iba_floam_map_register(H.p, pairs.data(), Ba, &mopt, sol.data())) return fail(h, s, who + H.p->err);
        // the map update: [old map, identity; scan cloud, T[k]], cropped around t[k], on the lattice
        std::vector<int32_t> fr(4 * (size_t)Ba);
        std::vector<double> poses(48 * (size_t)Ba);   // two sub-maps of two members per track, 12 doubles per member
        std::vector<iba_lattice_desc> descs(2 * (size_t)Ba);
        for (int a = 0; a < Ba; ++a) {
            const int b = act[(size_t)a];
            iba_floam_odom_step& s = R->tracks[(size_t)b].steps[(size_t)k];
            const iba_floam_map_result& r = sol[(size_t)a];
            std::memcpy(s.T_pred, pairs[(size_t)a].T, sizeof(s.T_pred)); std::memcpy(s.T, r.T, sizeof(s.T));
            s.initial_cost = r.initial_cost; s.final_cost = r.final_cost; s.passes = r.passes; s.iterations = r.iterations; s.evaluations = r.evaluations;
            s.n_edge = r.n_edge; s.n_surf = r.n_surf; s.status = r.status;
            for (int kind = 0; kind < 2; ++kind) {
                const size_t m = 2 * (size_t)a + kind;
                fr[2 * m] = 4 * a + 2 + kind; fr[2 * m + 1] = 4 * a + kind;
                std::memcpy(&poses[12 * (2 * m)], I12, sizeof(I12)); std::memcpy(&poses[12 * (2 * m + 1)], r.T, sizeof(I12));
                iba_lattice_desc& d = descs[m];
                odom_lattice_desc(d, 2, &fr[2 * m], &poses[12 * (2 * m)], res[kind]);
                d.has_crop = 1;
                for (int ax = 0; ax < 3; ++ax) { d.crop_lo[ax] = r.T[4 * ax + 3] - opt->crop_half; d.crop_hi[ax] = r.T[4 * ax + 3] + opt->crop_half; }
            }
        }
        iba_submap_clouds* c = nullptr;
        if (const iba_status s = vox_build(H.p, descs.data(), 2 * Ba, who, false, &c)) return fail(h, s, H.p->err);
        const std::unique_ptr<iba_submap_clouds> maps(c);
        d_map = H.p->vox.d_xyz.p;
        for (int a = 0; a < Ba; ++a) {
            const int b = act[(size_t)a];
            iba_floam_odom_step& s = R->tracks[(size_t)b].steps[(size_t)k];
            for (int kind = 0; kind < 2; ++kind) {
                map_off[2 * (size_t)b + kind] = maps->first[2 * (size_t)a + kind];
                map_cnt[2 * (size_t)b + kind] = maps->first[2 * (size_t)a + kind + 1] - maps->first[2 * (size_t)a + kind];
            }
            s.n_map_edge = map_cnt[2 * (size_t)b]; s.n_map_surf = map_cnt[2 * (size_t)b + 1];
            if (opt->keep_maps || k == tracks[b].n_scans - 1) HIP_TRY(h, keep_map(b, k, d_map, &map_off[2 * (size_t)b], &map_cnt[2 * (size_t)b]));
        }
        HIP_TRY(h, hipStreamSynchronize(st));   // the kept copies read H_k's buffer; H_k-1 goes, H_k stays for the next staging
        prev.reset(H.p); H.p = nullptr;
        map0.release();
    }

    // ---- the down-sampled clouds and the kept maps, down ----
    {
        const size_t nd = (size_t)ds->first[2 * (size_t)n];
        std::vector<double> hd(3 * nd);
        if (nd) HIP_TRY(h, hipMemcpyAsync(hd.data(), d_ds, sizeof(double) * 3 * nd, hipMemcpyDeviceToHost, st));
        std::vector<std::vector<double>> hk(kept.size());
        for (size_t m = 0; m < kept.size(); ++m) {
            hk[m].resize(3 * (kept[m].n[0] + kept[m].n[1]));
            if (!hk[m].empty()) HIP_TRY(h, hipMemcpyAsync(hk[m].data(), kept[m].xyz.p, sizeof(double) * hk[m].size(), hipMemcpyDeviceToHost, st));
        }
        HIP_TRY(h, hipStreamSynchronize(st));
        for (int b = 0; b < B; ++b)
            for (int k = 0; k < tracks[b].n_scans; ++k)
                for (int kind = 0; kind < 2; ++kind) {
                    const size_t sm = 2 * ((size_t)scan0[(size_t)b] + (size_t)k) + (size_t)kind;
                    odom_narrow(hd.data() + 3 * (size_t)ds->first[sm], (size_t)(ds->first[sm + 1] - ds->first[sm]), R->tracks[(size_t)b].src[kind][(size_t)k]);
                }
        for (size_t m = 0; m < kept.size(); ++m) {
            iba_floam_odom::Track& t = R->tracks[(size_t)kept[m].b];
            odom_narrow(hk[m].data(), kept[m].n[0], t.map[0][(size_t)kept[m].k]);
            odom_narrow(hk[m].data() + 3 * kept[m].n[0], kept[m].n[1], t.map[1][(size_t)kept[m].k]);
            t.has_map[(size_t)kept[m].k] = 1;
        }
    }
    *out = R.release();
    return IBA_OK;
}

int32_t iba_floam_odom_num(const iba_floam_odom* o) { return o ? (int32_t)o->tracks.size() : 0; }
int32_t iba_floam_odom_n_scans(const iba_floam_odom* o, int32_t b) { return (o && b >= 0 && b < (int32_t)o->tracks.size()) ? (int32_t)o->tracks[(size_t)b].steps.size() : -1; }
const iba_floam_odom_step* iba_floam_odom_steps(const iba_floam_odom* o, int32_t b) { return (o && b >= 0 && b < (int32_t)o->tracks.size()) ? o->tracks[(size_t)b].steps.data() : nullptr; }
const float* iba_floam_odom_src(const iba_floam_odom* o, int32_t b, int32_t k, int32_t kind, int64_t* n) {
    if (n) *n = -1;
    if (!o || b < 0 || b >= (int32_t)o->tracks.size() || kind < 0 || kind > 1) return nullptr;
    const iba_floam_odom::Track& t = o->tracks[(size_t)b];
    if (k < 0 || k >= (int32_t)t.steps.size()) return nullptr;
    if (n) *n = (int64_t)(t.src[kind][(size_t)k].size() / 3);
    return t.src[kind][(size_t)k].data();
}
const float* iba_floam_odom_map(const iba_floam_odom* o, int32_t b, int32_t k, int32_t kind, int64_t* n) {
    if (n) *n = -1;
    if (!o || b < 0 || b >= (int32_t)o->tracks.size() || kind < 0 || kind > 1) return nullptr;
    const iba_floam_odom::Track& t = o->tracks[(size_t)b];
    if (k < 0 || k >= (int32_t)t.steps.size() || !t.has_map[(size_t)k]) return nullptr;
    if (n) *n = (int64_t)(t.map[kind][(size_t)k].size() / 3);
    return t.map[kind][(size_t)k].data();
}
void iba_floam_odom_free(iba_floam_odom* o) { delete o; }
