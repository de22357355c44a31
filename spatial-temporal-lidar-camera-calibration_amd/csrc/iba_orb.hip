// ORB feature extraction (include/iba_mi355x.h, iba_orb_*): the C ABI, the result object and the launch chain of a call. The kernels are
// iba_orb_kernels.hpp, the host rules (plan, resize tables, quadtree distribution, arctangent, sine / cosine) iba_orb_host.hpp. A per-call unit
// (iba_call.hpp); the chain of a chunk of images: level 0 of every image up, the resize launches level by level, score, the cell count, the
// scan, the ordered cell write, the candidates down, O6 on the host, the keypoints up, orientation, blur, descriptor, the angles and descriptors down.
// The result keeps the keypoints on the host; with keep_stages it also owns each chunk's pyramid, score and blurred planes on the device.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cstdlib>
#include <cstring>
#include <string>
#include <thread>
#include <vector>

#include "../../include/iba_mi355x.h"
#include "../../include/iba_mi355x_debug.h"
#include "iba_call.hpp"
#include "iba_device_buf.hpp"
#include "iba_orb_host.hpp"
#include "iba_orb_kernels.hpp"
#include "iba_workers.hpp"

using iba::DevBuf;
using iba::PinnedBuf;
namespace orb = iba::orb;
using orb::OrbCell;
using orb::OrbKp;
using orb::OrbRow;
using orb::OrbTile;

namespace {

struct LevelRes {
    int32_t W = 0, H = 0;
    int32_t n_kp = 0, n_cand = 0, n_fallback = 0;
    size_t cand_base = 0;      // into the result's candidate arrays (keep_stages)
    uint64_t pix = 0;          // into the chunk's planes (keep_stages)
};
struct ImageRes {
    int32_t chunk = 0;
    size_t kp_base = 0; int32_t n_kp = 0;
    LevelRes lv[orb::kMaxLevels];
};
struct ChunkStage { DevBuf<uint8_t> pyr, score, blur; };

}  // namespace

struct iba_orb_features {
    int device = -1;                          // -1: a result without device buffers (iba_debug_orb_stub)
    iba_orb_options opt{};
    std::vector<ImageRes> img;
    std::vector<float> xy, angle, response, size;
    std::vector<int32_t> octave;
    std::vector<uint8_t> desc;
    std::vector<ChunkStage> stage;            // keep_stages: one per chunk
    std::vector<int32_t> cand_xy, cand_score; // keep_stages: every level's candidates in O5's order
    int32_t n_chunks = 0;
    float ms[7] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};   // IBA_ORB_TIMING (debug): resize, score, cell, host distribution with both copies, orientation, blur, descriptor
};

namespace {
thread_local iba::CallError t_err;

uint64_t pyramid_pixels(const orb::Plan& p) {
    uint64_t n = 0;
    for (int l = 0; l < p.L; ++l) n += (uint64_t)p.lv[l].W * (uint64_t)p.lv[l].H;
    return n;
}

int32_t tiles_x(int32_t W) { return (W + orb::kTileW - 1) / orb::kTileW; }
int32_t tiles_y(int32_t H) { return (H + orb::kTileH - 1) / orb::kTileH; }

// the tile table of some rows, in the order given
void push_tiles(std::vector<OrbTile>& tiles, int32_t row, int32_t W, int32_t H) {
    for (int32_t ty = 0; ty < tiles_y(H); ++ty)
        for (int32_t tx = 0; tx < tiles_x(W); ++tx) tiles.push_back(OrbTile{row, tx, ty, 0});
}

// one chunk: images a .. b of the call
iba_status run_chunk(iba_orb_features* res, const iba_orb_image* images, const std::vector<orb::Plan>& plans, int32_t a, int32_t b, int32_t chunk, bool timing) {
    const iba_orb_options& opt = res->opt;
    const int32_t L = opt.n_levels, nI = b - a;
    hipStream_t st = nullptr;
    // ---- the host arrays of the chain, its buffers, then the guard: it waits for the stream before any of them unwinds ----
    std::vector<OrbRow> rows((size_t)nI * (size_t)L);
    std::vector<OrbTile> tiles;
    std::vector<OrbCell> cells;
    std::vector<OrbKp> kps;
    std::vector<int32_t> tab, off, fb, cxy, cscore, row_kp;
    std::vector<float> ang;
    PinnedBuf<uint8_t> h_img;
    ChunkStage local;
    DevBuf<OrbRow> d_rows; DevBuf<OrbTile> d_tiles; DevBuf<int2> d_tab; DevBuf<OrbCell> d_cells;
    DevBuf<int32_t> d_cnt, d_fb, d_off, d_cscore, d_rowkp; DevBuf<int2> d_cxy;
    DevBuf<int8_t> d_pat;
    DevBuf<OrbKp> d_kps; DevBuf<float> d_ang; DevBuf<uint8_t> d_desc;
    iba::EventSet ev;
    iba::SyncOnExit sync(st);
    // ---- the tables ----
    std::vector<uint32_t> tile_level((size_t)L + 1, 0u);
    uint64_t pix = 0;
    for (int32_t l = 0; l < L; ++l) {
        tile_level[(size_t)l] = (uint32_t)tiles.size();
        for (int32_t i = 0; i < nI; ++i) {
            const orb::LevelPlan& v = plans[(size_t)(a + i)].lv[l];
            OrbRow& r = rows[(size_t)i * (size_t)L + (size_t)l];
            r.pix = pix; r.W = v.W; r.H = v.H; r.src = l > 0 ? i * L + l - 1 : -1; r.xtab = r.ytab = 0u; r.pad = 0;
            if (v.W < 1) continue;
            pix += (uint64_t)v.W * (uint64_t)v.H;
            push_tiles(tiles, i * L + l, v.W, v.H);
            if (l == 0) continue;
            const orb::LevelPlan& s = plans[(size_t)(a + i)].lv[l - 1];
            r.xtab = (uint32_t)(tab.size() / 2);
            tab.resize(tab.size() + 2 * (size_t)v.W);
            orb::resize_table(s.W, v.W, &tab[2 * (size_t)r.xtab]);
            r.ytab = (uint32_t)(tab.size() / 2);
            tab.resize(tab.size() + 2 * (size_t)v.H);
            orb::resize_table(s.H, v.H, &tab[2 * (size_t)r.ytab]);
        }
    }
    tile_level[(size_t)L] = (uint32_t)tiles.size();
    if (tiles.size() >= (1ull << 31) || tab.size() / 2 >= (1ull << 32)) return t_err.fail(IBA_ERR_UNSUPPORTED, "one chunk needs 2^31 blocks or more");
    std::vector<int32_t> row_cell((size_t)nI * (size_t)L + 1, 0);
    uint64_t cand_cap = 0;
    for (int32_t i = 0; i < nI; ++i)
        for (int32_t l = 0; l < L; ++l) {
            const orb::LevelPlan& v = plans[(size_t)(a + i)].lv[l];
            row_cell[(size_t)i * (size_t)L + (size_t)l] = (int32_t)cells.size();
            for (int32_t ci = 0; ci < v.nRows; ++ci)
                for (int32_t cj = 0; cj < v.nCols; ++cj) {
                    int32_t q[4];
                    if (!orb::cell_region(v, ci, cj, q)) continue;
                    if (q[1] - q[0] > orb::kCellMax || q[3] - q[2] > orb::kCellMax) return t_err.fail(IBA_ERR_UNSUPPORTED, "a cell wider than 59 pixels");
                    cells.push_back(OrbCell{i * L + l, q[0], q[1], q[2], q[3]});
                    cand_cap += (uint64_t)((q[1] - q[0] + 1) / 2) * (uint64_t)((q[3] - q[2] + 1) / 2);   // strict maxima of 3 x 3: at most one per 2 x 2
                }
        }
    row_cell[(size_t)nI * (size_t)L] = (int32_t)cells.size();
    const int32_t n_cells = (int32_t)cells.size();
    if (cand_cap >= (1ull << 31)) return t_err.fail(IBA_ERR_UNSUPPORTED, "one chunk may hold 2^31 candidates or more");
    // ---- the buffers ----
    ChunkStage& pl = opt.keep_stages ? res->stage[(size_t)chunk] : local;
    IBA_CALL_TRY(pl.pyr.alloc((size_t)pix)); IBA_CALL_TRY(pl.score.alloc((size_t)pix)); IBA_CALL_TRY(pl.blur.alloc((size_t)pix));
    IBA_CALL_TRY(d_rows.alloc(rows.size())); IBA_CALL_TRY(d_tiles.alloc(tiles.size())); IBA_CALL_TRY(d_tab.alloc(tab.size() / 2)); IBA_CALL_TRY(d_cells.alloc((size_t)n_cells));
    IBA_CALL_TRY(d_cnt.alloc((size_t)n_cells)); IBA_CALL_TRY(d_fb.alloc((size_t)n_cells)); IBA_CALL_TRY(d_off.alloc((size_t)n_cells + 1));
    IBA_CALL_TRY(d_cxy.alloc((size_t)cand_cap)); IBA_CALL_TRY(d_cscore.alloc((size_t)cand_cap)); IBA_CALL_TRY(d_rowkp.alloc(rows.size()));
    IBA_CALL_TRY(d_pat.alloc(1024));
    uint64_t n0 = 0;
    for (int32_t i = 0; i < nI; ++i) n0 += (uint64_t)images[a + i].W * (uint64_t)images[a + i].H;
    IBA_CALL_TRY(h_img.alloc((size_t)n0));
    {
        uint8_t* at = h_img.p;
        for (int32_t i = 0; i < nI; ++i) {
            const iba_orb_image& im = images[a + i];
            for (int32_t y = 0; y < im.H; ++y, at += im.W) std::memcpy(at, im.gray + (size_t)y * (size_t)im.stride, (size_t)im.W);
        }
    }
    if (timing) IBA_CALL_TRY(ev.create(8));
    IBA_CALL_TRY(hipMemcpyAsync(pl.pyr.p, h_img.p, (size_t)n0, hipMemcpyHostToDevice, st));
    IBA_CALL_TRY(hipMemcpyAsync(d_rows.p, rows.data(), sizeof(OrbRow) * rows.size(), hipMemcpyHostToDevice, st));
    IBA_CALL_TRY(hipMemcpyAsync(d_tiles.p, tiles.data(), sizeof(OrbTile) * tiles.size(), hipMemcpyHostToDevice, st));
    if (!tab.empty()) IBA_CALL_TRY(hipMemcpyAsync(d_tab.p, tab.data(), sizeof(int32_t) * tab.size(), hipMemcpyHostToDevice, st));
    if (n_cells) IBA_CALL_TRY(hipMemcpyAsync(d_cells.p, cells.data(), sizeof(OrbCell) * cells.size(), hipMemcpyHostToDevice, st));
    IBA_CALL_TRY(hipMemcpyAsync(d_pat.p, opt.pattern, 1024, hipMemcpyHostToDevice, st));
    IBA_CALL_TRY(hipMemsetAsync(pl.blur.p, 0, (size_t)pix, st));
    // ---- pyramid, scores, candidates ----
    if (timing) IBA_CALL_TRY(hipEventRecord(ev.e[0], st));
    for (int32_t l = 1; l < L; ++l) {
        const uint32_t nb = tile_level[(size_t)l + 1] - tile_level[(size_t)l];
        if (!nb) continue;
        hipLaunchKernelGGL(orb::orb_resize_kernel, dim3(nb), dim3(orb::kThreads), 0, st, d_rows.p, d_tiles.p + tile_level[(size_t)l], d_tab.p, pl.pyr.p);
        IBA_CALL_TRY(hipGetLastError());
    }
    if (timing) IBA_CALL_TRY(hipEventRecord(ev.e[1], st));
    hipLaunchKernelGGL(orb::orb_score_kernel, dim3((uint32_t)tiles.size()), dim3(orb::kThreads), 0, st, d_rows.p, d_tiles.p, pl.pyr.p, pl.score.p, (int)opt.min_th_fast);
    IBA_CALL_TRY(hipGetLastError());
    if (timing) IBA_CALL_TRY(hipEventRecord(ev.e[2], st));
    off.assign((size_t)n_cells + 1, 0); fb.assign((size_t)n_cells, 0);
    if (n_cells) {
        hipLaunchKernelGGL(orb::orb_cell_kernel<false>, dim3((uint32_t)n_cells), dim3(orb::kThreads), 0, st, d_rows.p, d_cells.p, pl.score.p, (int)opt.ini_th_fast, (int)opt.min_th_fast,
                           d_cnt.p, d_fb.p, (const int32_t*)nullptr, (int2*)nullptr, (int32_t*)nullptr);
        IBA_CALL_TRY(hipGetLastError());
        hipLaunchKernelGGL(orb::orb_scan_kernel, dim3(1), dim3(1024), 0, st, d_cnt.p, d_off.p, (int)n_cells);
        IBA_CALL_TRY(hipGetLastError());
        hipLaunchKernelGGL(orb::orb_cell_kernel<true>, dim3((uint32_t)n_cells), dim3(orb::kThreads), 0, st, d_rows.p, d_cells.p, pl.score.p, (int)opt.ini_th_fast, (int)opt.min_th_fast,
                           d_cnt.p, d_fb.p, d_off.p, d_cxy.p, d_cscore.p);
        IBA_CALL_TRY(hipGetLastError());
    }
    if (timing) IBA_CALL_TRY(hipEventRecord(ev.e[3], st));
    if (n_cells) {
        IBA_CALL_TRY(hipMemcpyAsync(off.data(), d_off.p, sizeof(int32_t) * off.size(), hipMemcpyDeviceToHost, st));
        IBA_CALL_TRY(hipMemcpyAsync(fb.data(), d_fb.p, sizeof(int32_t) * fb.size(), hipMemcpyDeviceToHost, st));
    }
    IBA_CALL_TRY(hipStreamSynchronize(st));
    const auto t_host0 = std::chrono::steady_clock::now();
    const int32_t n_cand = off[(size_t)n_cells];
    if (n_cand < 0 || (uint64_t)n_cand > cand_cap) return t_err.fail(IBA_ERR_STATE,"the cells kept more candidates than their bound");
    cxy.resize(2 * (size_t)n_cand); cscore.resize((size_t)n_cand);
    if (n_cand) {
        IBA_CALL_TRY(hipMemcpyAsync(cxy.data(), d_cxy.p, sizeof(int2) * (size_t)n_cand, hipMemcpyDeviceToHost, st));
        IBA_CALL_TRY(hipMemcpyAsync(cscore.data(), d_cscore.p, sizeof(int32_t) * (size_t)n_cand, hipMemcpyDeviceToHost, st));
        IBA_CALL_TRY(hipStreamSynchronize(st));
    }
    // ---- O6 on the host: every (image, level) on its own, on up to 16 threads when the chunk holds several images; the order of the output is fixed below ----
    std::vector<std::vector<int32_t>> chosen(rows.size());
    const auto distribute_row = [&](size_t ri) {
        const orb::LevelPlan& v = plans[(size_t)a + ri / (size_t)L].lv[ri % (size_t)L];
        if (v.nCols < 1) return;
        const int32_t k0 = off[(size_t)row_cell[ri]], k1 = off[(size_t)row_cell[ri + 1]];
        orb::distribute(cxy.data() + 2 * (size_t)k0, cscore.data() + k0, k1 - k0, v.W - 2 * orb::kMinB, v.H - 2 * orb::kMinB, v.n_features, chosen[ri]);
    };
    const int n_threads = (int)std::min<unsigned>(std::min<unsigned>(16u, (unsigned)nI), std::max(1u, std::thread::hardware_concurrency()));
    if (n_threads > 1) {
        std::atomic<size_t> next{0};
        iba::WorkerPool pool;
        pool.start(n_threads, nullptr);
        pool.run_all([&](int) { for (size_t ri; (ri = next.fetch_add(1)) < rows.size();) distribute_row(ri); return IBA_OK; });
        pool.stop();
    } else {
        for (size_t ri = 0; ri < rows.size(); ++ri) distribute_row(ri);
    }
    row_kp.assign(rows.size(), 0);
    for (int32_t i = 0; i < nI; ++i) {
        ImageRes& ir = res->img[(size_t)(a + i)];
        ir.chunk = chunk;
        ir.kp_base = res->octave.size() + kps.size();
        for (int32_t l = 0; l < L; ++l) {
            const size_t ri = (size_t)i * (size_t)L + (size_t)l;
            const orb::LevelPlan& v = plans[(size_t)(a + i)].lv[l];
            LevelRes& lr = ir.lv[l];
            lr.W = v.W; lr.H = v.H; lr.pix = rows[ri].pix;
            const int32_t ca = row_cell[ri], cb = row_cell[ri + 1];
            const int32_t k0 = off[(size_t)ca], k1 = off[(size_t)cb];
            lr.n_cand = k1 - k0;
            for (int32_t c = ca; c < cb; ++c) lr.n_fallback += fb[(size_t)c];
            if (opt.keep_stages) {
                lr.cand_base = res->cand_score.size();
                res->cand_xy.insert(res->cand_xy.end(), cxy.begin() + 2 * (size_t)k0, cxy.begin() + 2 * (size_t)k1);
                res->cand_score.insert(res->cand_score.end(), cscore.begin() + k0, cscore.begin() + k1);
            }
            lr.n_kp = (int32_t)chosen[ri].size();
            row_kp[ri] = lr.n_kp;
            for (const int32_t c : chosen[ri]) kps.push_back(OrbKp{(int32_t)ri, cxy[2 * (size_t)(k0 + c)] + orb::kMinB, cxy[2 * (size_t)(k0 + c) + 1] + orb::kMinB, cscore[(size_t)(k0 + c)]});
            ir.n_kp += lr.n_kp;
        }
    }
    const size_t nk = kps.size();
    ang.resize(nk);
    const size_t base = res->octave.size();
    res->desc.resize(32 * (base + nk));
    if (nk) {
        if (nk >= (1ull << 31)) return t_err.fail(IBA_ERR_UNSUPPORTED, "one chunk holds 2^31 keypoints or more");
        IBA_CALL_TRY(d_kps.alloc(nk)); IBA_CALL_TRY(d_ang.alloc(nk)); IBA_CALL_TRY(d_desc.alloc(32 * nk));
        IBA_CALL_TRY(hipMemcpyAsync(d_kps.p, kps.data(), sizeof(OrbKp) * nk, hipMemcpyHostToDevice, st));
        IBA_CALL_TRY(hipMemcpyAsync(d_rowkp.p, row_kp.data(), sizeof(int32_t) * row_kp.size(), hipMemcpyHostToDevice, st));
        const auto t_host1 = std::chrono::steady_clock::now();
        if (timing) res->ms[3] += std::chrono::duration<float, std::milli>(t_host1 - t_host0).count();
        orb::OrbUmax um;
        std::memcpy(um.u, plans[(size_t)a].umax, sizeof(um.u));
        if (timing) IBA_CALL_TRY(hipEventRecord(ev.e[4], st));
        hipLaunchKernelGGL(orb::orb_orient_kernel, dim3((uint32_t)((nk + 3) / 4)), dim3(orb::kThreads), 0, st, d_rows.p, d_kps.p, (int)nk, pl.pyr.p, um, d_ang.p);
        IBA_CALL_TRY(hipGetLastError());
        if (timing) IBA_CALL_TRY(hipEventRecord(ev.e[5], st));
        hipLaunchKernelGGL(orb::orb_blur_kernel, dim3((uint32_t)tiles.size()), dim3(orb::kThreads), 0, st, d_rows.p, d_tiles.p, d_rowkp.p, pl.pyr.p, pl.blur.p);
        IBA_CALL_TRY(hipGetLastError());
        if (timing) IBA_CALL_TRY(hipEventRecord(ev.e[6], st));
        hipLaunchKernelGGL(orb::orb_desc_kernel, dim3((uint32_t)((nk + 7) / 8)), dim3(orb::kThreads), 0, st, d_rows.p, d_kps.p, (int)nk, d_ang.p, pl.blur.p, (const char4*)d_pat.p, d_desc.p);
        IBA_CALL_TRY(hipGetLastError());
        if (timing) IBA_CALL_TRY(hipEventRecord(ev.e[7], st));
        IBA_CALL_TRY(hipMemcpyAsync(ang.data(), d_ang.p, sizeof(float) * nk, hipMemcpyDeviceToHost, st));
        IBA_CALL_TRY(hipMemcpyAsync(res->desc.data() + 32 * base, d_desc.p, 32 * nk, hipMemcpyDeviceToHost, st));
        IBA_CALL_TRY(hipStreamSynchronize(st));
    } else if (timing) {
        res->ms[3] += std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t_host0).count();
    }
    sync.disarm();                            // every copy of the chunk has been waited for
    if (timing) {
        const int pairs[6][3] = {{0, 1, 0}, {1, 2, 1}, {2, 3, 2}, {4, 5, 4}, {5, 6, 5}, {6, 7, 6}};
        for (const auto& p : pairs) {
            if (p[0] >= 4 && !nk) continue;
            float ms = 0.f;
            IBA_CALL_TRY(hipEventElapsedTime(&ms, ev.e[(size_t)p[0]], ev.e[(size_t)p[1]]));
            res->ms[p[2]] += ms;
        }
    }
    // ---- O10 ----
    for (size_t k = 0; k < nk; ++k) {
        const int32_t l = kps[k].row % L;
        const float sf = plans[(size_t)(a + kps[k].row / L)].lv[l].sf;
        res->xy.push_back((float)kps[k].x * sf); res->xy.push_back((float)kps[k].y * sf);
        res->angle.push_back(ang[k]);
        res->response.push_back((float)kps[k].score);
        res->octave.push_back(l);
        res->size.push_back((float)(int32_t)(31.f * sf));
    }
    return IBA_OK;
}

iba_status check_image_index(const iba_orb_features* f, int32_t image, const char* who) {
    return t_err.check_index(!f, image, f ? f->img.size() : 0, std::string(who) + ": ", "image");
}
iba_status check_stage(const iba_orb_features* f, int32_t image, int32_t level, const char* who) {
    if (const iba_status s = check_image_index(f, image, who)) return s;
    if (level < 0 || level >= f->opt.n_levels) return t_err.fail(IBA_ERR_INVALID_ARG, std::string(who) + ": level " + std::to_string(level) + " is outside the result's " + std::to_string(f->opt.n_levels) + " levels");
    if (!f->opt.keep_stages) return t_err.fail(IBA_ERR_INVALID_ARG, std::string(who) + ": the call did not ask for keep_stages");
    return IBA_OK;
}

}  // namespace

extern "C" {

const char* iba_orb_last_error(void) { return t_err.msg.c_str(); }

iba_status iba_default_orb_options(iba_orb_options* opt) {
    if (!opt) return t_err.fail(IBA_ERR_INVALID_ARG, "iba_default_orb_options: opt is NULL");
    std::memset(opt, 0, sizeof(*opt));
    opt->struct_size = (int32_t)sizeof(*opt);
    opt->n_features = 2000; opt->scale_factor = 1.2f; opt->n_levels = 8; opt->ini_th_fast = 20; opt->min_th_fast = 7;
    return IBA_OK;
}

iba_status iba_orb_plan(int32_t W, int32_t H, const iba_orb_options* opt, int32_t* level_wh, int32_t* features_per_level, int32_t* cells, int32_t* n_ini, int32_t umax[16]) {
    const std::string who = "iba_orb_plan: ";
    std::string why = orb::check_options(opt, false);
    if (!why.empty()) return t_err.fail(IBA_ERR_INVALID_ARG, who + why);
    orb::Plan p;
    why = orb::make_plan(W, H, *opt, p);
    if (!why.empty()) return t_err.fail(IBA_ERR_INVALID_ARG, who + why);
    for (int l = 0; l < p.L; ++l) {
        const orb::LevelPlan& v = p.lv[l];
        if (level_wh) { level_wh[2 * l] = v.W; level_wh[2 * l + 1] = v.H; }
        if (features_per_level) features_per_level[l] = v.n_features;
        if (cells) { cells[4 * l] = v.nCols; cells[4 * l + 1] = v.nRows; cells[4 * l + 2] = v.wCell; cells[4 * l + 3] = v.hCell; }
        if (n_ini) n_ini[l] = v.n_ini;
    }
    if (umax) std::memcpy(umax, p.umax, sizeof(p.umax));
    return IBA_OK;
}

iba_status iba_orb_distribute(const int32_t* xy, const int32_t* score, int32_t n, int32_t width, int32_t height, int32_t N, int32_t* chosen, int32_t* n_chosen) {
    const std::string who = "iba_orb_distribute: ";
    if (n_chosen) *n_chosen = 0;
    if (!n_chosen || n < 0 || (n > 0 && (!xy || !score || !chosen))) return t_err.fail(IBA_ERR_INVALID_ARG, who + "a NULL argument or n < 0");
    if (width < 1 || height < 1 || N < 0) return t_err.fail(IBA_ERR_INVALID_ARG, who + "width < 1, height < 1 or N < 0");
    if ((int32_t)std::round((float)width / (float)height) < 1) return t_err.fail(IBA_ERR_INVALID_ARG, who + "no start node: round(width / height) is 0");
    for (int32_t k = 0; k < n; ++k)
        if (xy[2 * k] < 0 || xy[2 * k] >= width || xy[2 * k + 1] < 0 || xy[2 * k + 1] >= height) return t_err.fail(IBA_ERR_INVALID_ARG, who + "candidate " + std::to_string(k) + " lies outside width x height");
    std::vector<int32_t> out;
    orb::distribute(xy, score, n, width, height, N, out);
    for (size_t k = 0; k < out.size(); ++k) chosen[k] = out[k];
    *n_chosen = (int32_t)out.size();
    return IBA_OK;
}

iba_status iba_orb_extract(const iba_orb_image* images, int32_t n, const iba_orb_options* opt, int device, iba_orb_features** out) {
    const std::string who = "iba_orb_extract: ";
    if (out) *out = nullptr;
    if (!out) return t_err.fail(IBA_ERR_INVALID_ARG, who + "out is NULL");
    if (!images) return t_err.fail(IBA_ERR_INVALID_ARG, who + "images is NULL");
    if (n < 1) return t_err.fail(IBA_ERR_INVALID_ARG, who + "n < 1");
    std::string why = orb::check_options(opt, true);
    if (!why.empty()) return t_err.fail(IBA_ERR_INVALID_ARG, who + why);
    std::vector<orb::Plan> plans((size_t)n);
    std::vector<uint64_t> bytes((size_t)n);
    for (int32_t i = 0; i < n; ++i) {
        const iba_orb_image& im = images[i];
        if (!im.gray) return t_err.fail(IBA_ERR_INVALID_ARG, who + "image " + std::to_string(i) + ": gray is NULL");
        if (im.W < 1 || im.H < 1 || im.stride < (int64_t)im.W) return t_err.fail(IBA_ERR_INVALID_ARG, who + "image " + std::to_string(i) + ": W < 1, H < 1 or stride < W");
        why = orb::make_plan(im.W, im.H, *opt, plans[(size_t)i]);
        if (!why.empty()) return t_err.fail(IBA_ERR_INVALID_ARG, who + "image " + std::to_string(i) + ": " + why);
        bytes[(size_t)i] = IBA_ORB_BYTES_PER_PIXEL * pyramid_pixels(plans[(size_t)i]);
    }
    // ---- the device from here on ----
    uint64_t budget = 0;
    IBA_CALL_TRY(iba::call_budget(device, IBA_ORB_BUDGET_BYTES, "IBA_ORB_BUDGET", &budget));
    const bool timing = iba::debug_env("IBA_ORB_TIMING") != nullptr;
    const std::vector<int32_t> cut = iba::cut_chunks(bytes, budget);
    iba_orb_features* res = new iba_orb_features();
    res->device = device; res->opt = *opt;   // (the pattern is read during the call only)
    res->img.resize((size_t)n);
    res->n_chunks = (int32_t)cut.size() - 1;
    if (opt->keep_stages) res->stage.resize((size_t)res->n_chunks);
    iba_status s = IBA_OK;
    for (int32_t c = 0; c < res->n_chunks && s == IBA_OK; ++c) s = run_chunk(res, images, plans, cut[(size_t)c], cut[(size_t)c + 1], c, timing);
    res->opt.pattern = nullptr;
    if (s != IBA_OK) { t_err.msg = who + t_err.msg; delete res; return s; }
    *out = res;
    return IBA_OK;
}

void iba_orb_free(iba_orb_features* f) {
    if (!f) return;
    if (f->device >= 0) (void)hipSetDevice(f->device);
    delete f;
}

int32_t iba_orb_n_images(const iba_orb_features* f) { return f ? (int32_t)f->img.size() : 0; }

iba_status iba_orb_counts(const iba_orb_features* f, int32_t image, int32_t* n_keypoints, int32_t* per_level, int32_t* candidates_per_level, int32_t* fallback_cells_per_level) {
    if (const iba_status s = check_image_index(f, image, "iba_orb_counts")) return s;
    const ImageRes& ir = f->img[(size_t)image];
    if (n_keypoints) *n_keypoints = ir.n_kp;
    for (int32_t l = 0; l < f->opt.n_levels; ++l) {
        if (per_level) per_level[l] = ir.lv[l].n_kp;
        if (candidates_per_level) candidates_per_level[l] = ir.lv[l].n_cand;
        if (fallback_cells_per_level) fallback_cells_per_level[l] = ir.lv[l].n_fallback;
    }
    return IBA_OK;
}

iba_status iba_orb_read(iba_orb_features* f, int32_t image, float* xy, float* angle, float* response, int32_t* octave, float* size, uint8_t* desc) {
    if (const iba_status s = check_image_index(f, image, "iba_orb_read")) return s;
    const ImageRes& ir = f->img[(size_t)image];
    const size_t b = ir.kp_base, n = (size_t)ir.n_kp;
    if (!n) return IBA_OK;
    if (xy) std::memcpy(xy, &f->xy[2 * b], sizeof(float) * 2 * n);
    if (angle) std::memcpy(angle, &f->angle[b], sizeof(float) * n);
    if (response) std::memcpy(response, &f->response[b], sizeof(float) * n);
    if (octave) std::memcpy(octave, &f->octave[b], sizeof(int32_t) * n);
    if (size) std::memcpy(size, &f->size[b], sizeof(float) * n);
    if (desc) std::memcpy(desc, &f->desc[32 * b], 32 * n);
    return IBA_OK;
}

iba_status iba_orb_level(iba_orb_features* f, int32_t image, int32_t level, int32_t blurred, uint8_t* out) {
    if (const iba_status s = check_stage(f, image, level, "iba_orb_level")) return s;
    if (!out) return t_err.fail(IBA_ERR_INVALID_ARG, "iba_orb_level: the output is NULL");
    const ImageRes& ir = f->img[(size_t)image];
    const LevelRes& lr = ir.lv[level];
    const size_t bytes = (size_t)lr.W * (size_t)lr.H;
    if (f->device < 0 || !bytes) return IBA_OK;
    IBA_CALL_TRY(hipSetDevice(f->device));
    const ChunkStage& cs = f->stage[(size_t)ir.chunk];
    IBA_CALL_TRY(hipMemcpy(out, (blurred ? cs.blur.p : cs.pyr.p) + lr.pix, bytes, hipMemcpyDeviceToHost));
    return IBA_OK;
}

iba_status iba_orb_scores(iba_orb_features* f, int32_t image, int32_t level, uint8_t* out) {
    if (const iba_status s = check_stage(f, image, level, "iba_orb_scores")) return s;
    if (!out) return t_err.fail(IBA_ERR_INVALID_ARG, "iba_orb_scores: the output is NULL");
    const ImageRes& ir = f->img[(size_t)image];
    const LevelRes& lr = ir.lv[level];
    const size_t bytes = (size_t)lr.W * (size_t)lr.H;
    if (f->device < 0 || !bytes) return IBA_OK;
    IBA_CALL_TRY(hipSetDevice(f->device));
    IBA_CALL_TRY(hipMemcpy(out, f->stage[(size_t)ir.chunk].score.p + lr.pix, bytes, hipMemcpyDeviceToHost));
    return IBA_OK;
}

iba_status iba_orb_candidates(iba_orb_features* f, int32_t image, int32_t level, int32_t* xy, int32_t* score) {
    if (const iba_status s = check_stage(f, image, level, "iba_orb_candidates")) return s;
    const LevelRes& lr = f->img[(size_t)image].lv[level];
    if (!lr.n_cand) return IBA_OK;
    if (xy) std::memcpy(xy, &f->cand_xy[2 * lr.cand_base], sizeof(int32_t) * 2 * (size_t)lr.n_cand);
    if (score) std::memcpy(score, &f->cand_score[lr.cand_base], sizeof(int32_t) * (size_t)lr.n_cand);
    return IBA_OK;
}

// ---- debug (include/iba_mi355x_debug.h) ----

float iba_debug_orb_atan2(float y, float x) { return orb::orb_atan2_deg(y, x); }

iba_status iba_debug_orb_sincos(float angle_deg, float ab[2], double cs[2]) {
    if (!ab || !cs) return t_err.fail(IBA_ERR_INVALID_ARG, "iba_debug_orb_sincos: a NULL argument");
    const float a_rad = angle_deg * (float)(3.14159265358979323846 / 180.0);
    orb::orb_sincos((double)a_rad, &cs[0], &cs[1]);
    orb::orb_angle_ab(angle_deg, &ab[0], &ab[1]);
    return IBA_OK;
}

iba_status iba_debug_orb_stub(int32_t n_images, int32_t n_levels, int32_t keep_stages, iba_orb_features** out) {
    if (!out || n_images < 0 || n_levels < 1 || n_levels > orb::kMaxLevels) return t_err.fail(IBA_ERR_INVALID_ARG, "iba_debug_orb_stub: out is NULL, n_images < 0 or n_levels outside 1..16");
    iba_orb_features* res = new iba_orb_features();
    (void)iba_default_orb_options(&res->opt);
    res->opt.n_levels = n_levels; res->opt.keep_stages = keep_stages ? 1 : 0;
    res->img.resize((size_t)n_images);
    *out = res;
    return IBA_OK;
}

int32_t iba_debug_orb_chunks(const iba_orb_features* f) { return f ? f->n_chunks : 0; }

iba_status iba_debug_orb_stage_ms(const iba_orb_features* f, float ms[7]) {
    if (!f || !ms) return t_err.fail(IBA_ERR_INVALID_ARG, "iba_debug_orb_stage_ms: a NULL argument");
    std::memcpy(ms, f->ms, sizeof(f->ms));
    return IBA_OK;
}

iba_status iba_debug_orb_describe(const uint8_t* gray, int32_t W, int32_t H, const int32_t* xy, const float* angle, int32_t n, const int8_t* pattern, int device, uint8_t* blurred, uint8_t* desc) {
    const std::string who = "iba_debug_orb_describe: ";
    if (!gray || !xy || !angle || !pattern || !desc || n < 1) return t_err.fail(IBA_ERR_INVALID_ARG, who + "a NULL argument or n < 1");
    if (W < 2 * orb::kEdge + 1 || H < 2 * orb::kEdge + 1) return t_err.fail(IBA_ERR_INVALID_ARG, who + "the image is smaller than 39 x 39");
    for (int i = 0; i < 512; ++i)
        if ((int)pattern[2 * i] * pattern[2 * i] + (int)pattern[2 * i + 1] * pattern[2 * i + 1] > 324) return t_err.fail(IBA_ERR_INVALID_ARG, who + "a pattern point outside the disc of radius 18");
    std::vector<OrbKp> kps((size_t)n);
    for (int32_t k = 0; k < n; ++k) {
        const int32_t x = xy[2 * k], y = xy[2 * k + 1];
        if (x < orb::kEdge || x >= W - orb::kEdge || y < orb::kEdge || y >= H - orb::kEdge) return t_err.fail(IBA_ERR_INVALID_ARG, who + "keypoint " + std::to_string(k) + " lies within 19 pixels of the edge");
        if (!std::isfinite(angle[k]) || angle[k] < -720.f || angle[k] > 720.f) return t_err.fail(IBA_ERR_INVALID_ARG, who + "an angle outside -720..720");
        kps[(size_t)k] = OrbKp{0, x, y, 0};
    }
    IBA_CALL_TRY(hipSetDevice(device));
    OrbRow row{0, W, H, -1, 0u, 0u, 0};
    std::vector<OrbTile> tiles;
    push_tiles(tiles, 0, W, H);
    const int32_t one = 1;
    const size_t px = (size_t)W * (size_t)H;
    DevBuf<OrbRow> d_row; DevBuf<OrbTile> d_tiles; DevBuf<int32_t> d_one; DevBuf<uint8_t> d_img, d_blur, d_desc; DevBuf<OrbKp> d_kps; DevBuf<float> d_ang; DevBuf<int8_t> d_pat;
    IBA_CALL_TRY(d_row.upload(&row, 1)); IBA_CALL_TRY(d_tiles.upload(tiles)); IBA_CALL_TRY(d_one.upload(&one, 1)); IBA_CALL_TRY(d_img.upload(gray, px)); IBA_CALL_TRY(d_blur.alloc(px));
    IBA_CALL_TRY(d_kps.upload(kps)); IBA_CALL_TRY(d_ang.upload(angle, (size_t)n)); IBA_CALL_TRY(d_pat.upload(pattern, 1024)); IBA_CALL_TRY(d_desc.alloc(32 * (size_t)n));
    hipLaunchKernelGGL(orb::orb_blur_kernel, dim3((uint32_t)tiles.size()), dim3(orb::kThreads), 0, nullptr, d_row.p, d_tiles.p, d_one.p, d_img.p, d_blur.p);
    IBA_CALL_TRY(hipGetLastError());
    hipLaunchKernelGGL(orb::orb_desc_kernel, dim3((uint32_t)((n + 7) / 8)), dim3(orb::kThreads), 0, nullptr, d_row.p, d_kps.p, (int)n, d_ang.p, d_blur.p, (const char4*)d_pat.p, d_desc.p);
    IBA_CALL_TRY(hipGetLastError());
    if (blurred) IBA_CALL_TRY(hipMemcpy(blurred, d_blur.p, px, hipMemcpyDeviceToHost));
    IBA_CALL_TRY(hipMemcpy(desc, d_desc.p, 32 * (size_t)n, hipMemcpyDeviceToHost));
    return IBA_OK;
}

}  // extern "C"
