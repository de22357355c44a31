// ORB extraction, the host half (include/iba_mi355x.h, rules O1-O10): the plan of an image (levels, features per level, cells, start nodes, umax),
// the resize tables, the quadtree distribution, the arctangent polynomial and the f64 sine / cosine pair. No device code and no HIP type: the
// sanitizer self-test compiles this file with plain g++. The two functions the kernels share (orb_atan2_deg, orb_sincos) are marked IBA_ORB_HD.
#pragma once
#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <list>
#include <string>
#include <utility>
#include <vector>

#include "../../include/iba_mi355x.h"

#if defined(__HIPCC__)
#define IBA_ORB_HD __host__ __device__
#else
#define IBA_ORB_HD
#endif

namespace iba {
namespace orb {

constexpr int kMaxLevels = 16;
constexpr int kEdge = 19;        // EDGE_THRESHOLD: keypoints lie at least this far from a level's edge
constexpr int kMinB = 16;        // EDGE_THRESHOLD - 3: the border of the FAST region
constexpr int kHalfPatch = 15;   // HALF_PATCH_SIZE

// O7: the degree arctangent polynomial (float32, every operation rounded; the library is built without contraction)
IBA_ORB_HD inline float orb_atan2_deg(float y, float x) {
    const float scale = (float)(180.0 / 3.14159265358979323846);
    const float p1 = 0.9997878412794807f * scale, p3 = -0.3258083974640975f * scale, p5 = 0.1555786518463281f * scale, p7 = -0.04432655554792128f * scale;
    const float ax = x < 0.f ? -x : x, ay = y < 0.f ? -y : y;
    float a, c, c2;
    if (ax >= ay) {
        c = ay / (ax + (float)DBL_EPSILON);
        c2 = c * c;
        a = (((p7 * c2 + p5) * c2 + p3) * c2 + p1) * c;
    } else {
        c = ax / (ay + (float)DBL_EPSILON);
        c2 = c * c;
        a = 90.f - (((p7 * c2 + p5) * c2 + p3) * c2 + p1) * c;
    }
    if (x < 0.f) a = 180.f - a;
    if (y < 0.f) a = 360.f - a;
    return a;
}

// O9: cosine and sine of x (radians, |x| < 2^20) from one fixed sequence of f64 operations: q = floor(x * 2/pi + 0.5), r = (x - q * pio2_hi) - q * pio2_lo,
// the two kernels' polynomials in Horner form, the quadrant swap. tests/orb_ref.py mirrors it operation by operation.
IBA_ORB_HD inline void orb_sincos(double x, double* c_out, double* s_out) {
    const double two_over_pi = 6.36619772367581382433e-01, pio2_hi = 1.57079632673412561417e+00, pio2_lo = 6.07710050650619224932e-11;
    const double q = floor(x * two_over_pi + 0.5);
    const double r = (x - q * pio2_hi) - q * pio2_lo;
    const double z = r * r;
    const double S1 = -1.66666666666666324348e-01, S2 = 8.33333333332248946124e-03, S3 = -1.98412698298579493134e-04, S4 = 2.75573137070700676789e-06,
                 S5 = -2.50507602534068634195e-08, S6 = 1.58969099521155010221e-10;
    const double C1 = 4.16666666666666019037e-02, C2 = -1.38888888888741095749e-03, C3 = 2.48015872894767294178e-05, C4 = -2.75573143513906633035e-07,
                 C5 = 2.08757232129817482790e-09, C6 = -1.13596475577881948265e-11;
    const double ps = S1 + z * (S2 + z * (S3 + z * (S4 + z * (S5 + z * S6))));
    const double pc = C1 + z * (C2 + z * (C3 + z * (C4 + z * (C5 + z * C6))));
    const double s = r + (r * z) * ps;
    const double c = (1.0 - 0.5 * z) + (z * z) * pc;
    const int k = (int)((long long)q & 3);
    *c_out = k == 0 ? c : k == 1 ? -s : k == 2 ? -c : s;
    *s_out = k == 0 ? s : k == 1 ? c : k == 2 ? -s : -c;
}

// the float pair (a = cos, b = sin) of a keypoint's angle in degrees
IBA_ORB_HD inline void orb_angle_ab(float angle_deg, float* a, float* b) {
    const float a_rad = angle_deg * (float)(3.14159265358979323846 / 180.0);
    double c, s;
    orb_sincos((double)a_rad, &c, &s);
    *a = (float)c; *b = (float)s;
}

struct LevelPlan {
    int32_t W = 0, H = 0;              // 0 0: an empty level
    int32_t n_features = 0;
    int32_t nCols = 0, nRows = 0, wCell = 0, hCell = 0;   // zeros: the level has no cells
    int32_t n_ini = 0;
    float sf = 1.f;
};
struct Plan {
    int32_t L = 0;
    LevelPlan lv[kMaxLevels];
    int32_t umax[16];
};

inline std::string check_options(const iba_orb_options* o, bool need_pattern) {
    if (!o) return "opt is NULL";
    if (o->struct_size != (int32_t)sizeof(iba_orb_options)) return "opt->struct_size is " + std::to_string(o->struct_size) + ", not " + std::to_string(sizeof(iba_orb_options));
    if (o->n_features < 1) return "n_features < 1";
    if (!std::isfinite(o->scale_factor) || !(o->scale_factor > 1.f)) return "scale_factor must be finite and > 1";
    if (o->n_levels < 1 || o->n_levels > kMaxLevels) return "n_levels outside 1..16";
    if (o->min_th_fast < 1 || o->min_th_fast > o->ini_th_fast || o->ini_th_fast > 254) return "the thresholds must satisfy 1 <= min_th_fast <= ini_th_fast <= 254";
    if (o->keep_stages != 0 && o->keep_stages != 1) return "keep_stages must be 0 or 1";
    if (!need_pattern) return "";
    if (!o->pattern) return "pattern is NULL (the library ships no test-pair table: pass 256 x 4 int8)";
    for (int i = 0; i < 512; ++i) {
        const int x = o->pattern[2 * i], y = o->pattern[2 * i + 1];
        if (x * x + y * y > 324) return "pattern point " + std::to_string(i) + " lies outside the disc of radius 18";
    }
    return "";
}

// O1, O3, the start nodes of O6 and umax of O7 for one image size; "" or the refusal
inline std::string make_plan(int32_t W, int32_t H, const iba_orb_options& o, Plan& p) {
    if (W < 1 || H < 1) return "an image with W < 1 or H < 1";
    p.L = o.n_levels;
    float sf = 1.f;
    const float factor = 1.0f / o.scale_factor;
    float desired = (float)o.n_features * (1.f - factor) / (1.f - (float)std::pow((double)factor, (double)o.n_levels));
    int32_t sum = 0;
    for (int l = 0; l < p.L; ++l) {
        LevelPlan& v = p.lv[l];
        v = LevelPlan();
        if (l > 0) sf = sf * o.scale_factor;
        v.sf = sf;
        const float inv = 1.0f / sf;
        const float wf = (float)W * inv, hf = (float)H * inv;
        const int32_t Wl = std::isfinite(wf) && wf < 2.0e9f ? (int32_t)std::nearbyint(wf) : 0, Hl = std::isfinite(hf) && hf < 2.0e9f ? (int32_t)std::nearbyint(hf) : 0;
        if (Wl >= 1 && Hl >= 1) { v.W = Wl; v.H = Hl; }
        if (l < p.L - 1) {
            v.n_features = (int32_t)std::nearbyint(desired);
            sum += v.n_features;
            desired *= factor;
        } else {
            v.n_features = std::max(o.n_features - sum, 0);
        }
        const int32_t width = v.W - 2 * kMinB, height = v.H - 2 * kMinB;
        const int32_t nCols = width / 30, nRows = height / 30;
        if (width < 30 || height < 30 || nCols < 1 || nRows < 1) continue;
        v.nCols = nCols; v.nRows = nRows;
        v.wCell = (int32_t)std::ceil((float)width / (float)nCols);
        v.hCell = (int32_t)std::ceil((float)height / (float)nRows);
        v.n_ini = (int32_t)std::round((float)width / (float)height);
        if (v.n_ini < 1) return "level " + std::to_string(l) + " (" + std::to_string(v.W) + " x " + std::to_string(v.H) + ") has cells but no start node: round(width / height) is 0";
    }
    // umax: the end of each row of the circular patch
    const int vmax = (int)std::floor((float)kHalfPatch * std::sqrt(2.f) / 2 + 1), vmin = (int)std::ceil((float)kHalfPatch * std::sqrt(2.f) / 2);
    const double hp2 = (double)(kHalfPatch * kHalfPatch);
    for (int v = 0; v < 16; ++v) p.umax[v] = 0;
    for (int v = 0; v <= vmax; ++v) p.umax[v] = (int32_t)std::nearbyint(std::sqrt(hp2 - (double)(v * v)));
    for (int v = kHalfPatch, v0 = 0; v >= vmin; --v) {
        while (p.umax[v0] == p.umax[v0 + 1]) ++v0;
        p.umax[v] = v0;
        ++v0;
    }
    return "";
}

// the tested region of cell (i, j) of a level in level pixels: [x0, x1) x [y0, y1); false when it is empty (such a cell does not exist)
inline bool cell_region(const LevelPlan& v, int i, int j, int32_t r[4]) {
    const int32_t maxBX = v.W - kMinB, maxBY = v.H - kMinB;
    const int32_t iniY = kMinB + i * v.hCell, iniX = kMinB + j * v.wCell;
    const int32_t maxY = std::min(iniY + v.hCell + 6, maxBY), maxX = std::min(iniX + v.wCell + 6, maxBX);
    if (iniY >= maxBY - 3 || iniX >= maxBX - 6) return false;
    r[0] = iniX + 3; r[1] = maxX - 3; r[2] = iniY + 3; r[3] = maxY - 3;
    return r[0] < r[1] && r[2] < r[3];
}

// O2: the index and coefficient table of one axis: tab[2 d] = s, tab[2 d + 1] = c1 (c0 = 2048 - c1)
inline void resize_table(int32_t src, int32_t dst, int32_t* tab) {
    const double scale = (double)src / (double)dst;
    for (int32_t d = 0; d < dst; ++d) {
        float f = (float)(((double)d + 0.5) * scale - 0.5);
        int32_t s = (int32_t)std::floor(f);
        f -= (float)s;
        if (s < 0) { s = 0; f = 0.f; }
        if (s >= src - 1) { s = src - 1; f = 0.f; }
        tab[2 * d] = s;
        tab[2 * d + 1] = (int32_t)(int16_t)std::nearbyint(f * 2048.f);
    }
}

// O6: DistributeOctTree / DivideNode on integer candidates. chosen receives candidate indices in the order of the node list.
struct Node {
    int32_t ULx, ULy, URx, URy, BLx, BLy, BRx, BRy;
    std::vector<int32_t> keys;
    bool no_more = false;
    uint64_t seq = 0;                       // creation order: the tie rule of the second phase
    std::list<Node>::iterator lit;
};

inline void divide_node(const Node& n, const int32_t* xy, Node c[4]) {
    const int32_t halfX = (int32_t)std::ceil((float)(n.URx - n.ULx) / 2), halfY = (int32_t)std::ceil((float)(n.BRy - n.ULy) / 2);
    c[0].ULx = n.ULx; c[0].ULy = n.ULy; c[0].URx = n.ULx + halfX; c[0].URy = n.ULy;
    c[0].BLx = n.ULx; c[0].BLy = n.ULy + halfY; c[0].BRx = n.ULx + halfX; c[0].BRy = n.ULy + halfY;
    c[1].ULx = c[0].URx; c[1].ULy = c[0].URy; c[1].URx = n.URx; c[1].URy = n.URy;
    c[1].BLx = c[0].BRx; c[1].BLy = c[0].BRy; c[1].BRx = n.URx; c[1].BRy = n.ULy + halfY;
    c[2].ULx = c[0].BLx; c[2].ULy = c[0].BLy; c[2].URx = c[0].BRx; c[2].URy = c[0].BRy;
    c[2].BLx = n.BLx; c[2].BLy = n.BLy; c[2].BRx = c[0].BRx; c[2].BRy = n.BLy;
    c[3].ULx = c[2].URx; c[3].ULy = c[2].URy; c[3].URx = c[1].BRx; c[3].URy = c[1].BRy;
    c[3].BLx = c[2].BRx; c[3].BLy = c[2].BRy; c[3].BRx = n.BRx; c[3].BRy = n.BRy;
    for (const int32_t k : n.keys) {
        const int32_t x = xy[2 * k], y = xy[2 * k + 1];
        if (x < c[0].URx) c[y < c[0].BRy ? 0 : 2].keys.push_back(k);
        else c[y < c[0].BRy ? 1 : 3].keys.push_back(k);
    }
    for (int q = 0; q < 4; ++q) c[q].no_more = c[q].keys.size() == 1;
}

struct DistributeStats { int32_t phase2 = 0, size_tie = 0; };

inline void distribute(const int32_t* xy, const int32_t* score, int32_t n, int32_t width, int32_t height, int32_t N, std::vector<int32_t>& chosen, DistributeStats* stats = nullptr) {
    chosen.clear();
    const int32_t n_ini = (int32_t)std::round((float)width / (float)height);
    if (n_ini < 1 || n < 1) return;
    const float hX = (float)width / (float)n_ini;
    std::list<Node> nodes;
    std::vector<Node*> ini((size_t)n_ini);
    uint64_t seq = 0;
    for (int32_t i = 0; i < n_ini; ++i) {
        Node ni;
        ni.ULx = (int32_t)(hX * (float)i); ni.ULy = 0;
        ni.URx = (int32_t)(hX * (float)(i + 1)); ni.URy = 0;
        ni.BLx = ni.ULx; ni.BLy = height; ni.BRx = ni.URx; ni.BRy = height;
        ni.seq = seq++;
        nodes.push_back(ni);
        ini[(size_t)i] = &nodes.back();
    }
    for (int32_t k = 0; k < n; ++k) {
        const int32_t at = std::min(std::max((int32_t)((float)xy[2 * k] / hX), 0), n_ini - 1);
        ini[(size_t)at]->keys.push_back(k);
    }
    for (auto it = nodes.begin(); it != nodes.end();) {
        if (it->keys.size() == 1) { it->no_more = true; ++it; }
        else if (it->keys.empty()) it = nodes.erase(it);
        else ++it;
    }
    typedef std::pair<int32_t, Node*> SizeNode;
    std::vector<SizeNode> expand;
    const auto by_size_then_age = [](const SizeNode& a, const SizeNode& b) { return a.first != b.first ? a.first < b.first : a.second->seq < b.second->seq; };
    // the children of *parent to the front of the list, n1..n4; those with more than one key are recorded
    const auto push_children = [&](const Node& parent, int32_t* n_expand) {
        Node c[4];
        divide_node(parent, xy, c);
        for (int q = 0; q < 4; ++q) {
            if (c[q].keys.empty()) continue;
            c[q].seq = seq++;
            nodes.push_front(std::move(c[q]));
            if (nodes.front().keys.size() > 1) {
                if (n_expand) ++*n_expand;
                expand.push_back(SizeNode((int32_t)nodes.front().keys.size(), &nodes.front()));
                nodes.front().lit = nodes.begin();
            }
        }
    };
    bool finish = false;
    while (!finish) {
        int32_t prev = (int32_t)nodes.size(), n_expand = 0;
        expand.clear();
        for (auto it = nodes.begin(); it != nodes.end();) {
            if (it->no_more) { ++it; continue; }
            push_children(*it, &n_expand);
            it = nodes.erase(it);
        }
        if ((int32_t)nodes.size() >= N || (int32_t)nodes.size() == prev) {
            finish = true;
        } else if ((int32_t)nodes.size() + n_expand * 3 > N) {
            if (stats) stats->phase2 = 1;
            while (!finish) {
                prev = (int32_t)nodes.size();
                std::vector<SizeNode> todo = expand;
                expand.clear();
                std::sort(todo.begin(), todo.end(), by_size_then_age);
                for (size_t j = 1; stats && j < todo.size(); ++j) if (todo[j].first == todo[j - 1].first) stats->size_tie = 1;
                for (int32_t j = (int32_t)todo.size() - 1; j >= 0; --j) {
                    push_children(*todo[(size_t)j].second, nullptr);
                    nodes.erase(todo[(size_t)j].second->lit);
                    if ((int32_t)nodes.size() >= N) break;
                }
                if ((int32_t)nodes.size() >= N || (int32_t)nodes.size() == prev) finish = true;
            }
        }
    }
    for (const Node& nd : nodes) {
        int32_t best = nd.keys[0];
        for (size_t k = 1; k < nd.keys.size(); ++k) if (score[nd.keys[k]] > score[best]) best = nd.keys[k];
        chosen.push_back(best);
    }
}

}  // namespace orb
}  // namespace iba
