// Bundle adjustment, the arithmetic of rules B1-B10 (include/iba_mi355x.h, iba_bundle*): ONE text for the kernels (iba_bundle_kernels.hpp), the host
// restatement (iba_bundle_host.hpp) and the stand-alone sanitizer self-test, which compiles this file with plain g++. Every function here is the work
// of ONE item (an edge, a point, a lane of a camera's wave, a lane of a block's wave, a job's one sequencing lane) over the flat tables of a chunk of
// jobs (Tab); the kernels give the items to lanes, the host restatement walks them in loops. The edge, the Huber kernel, the pose update and the
// canonical NaN are iba_pose_math.hpp's. float64, every operation rounded, left to right as written, no contraction.
#pragma once
#include <cmath>
#include <cstdint>

#include "iba_pose_math.hpp"

#if defined(__clang__)
#pragma clang fp contract(off)
#endif

namespace iba {
namespace bundle {

constexpr int kMaxRounds = 4;
constexpr int kMaxFree = 64;                // IBA_BUNDLE_MAX_FREE_CAMERAS
constexpr int kMaxReduced = 6 * kMaxFree;
constexpr int kWave = 64;                   // B3: the lanes of a camera's and of a block's sums
constexpr int kLanes = 256;                 // B3: the lanes of a job's chi2
constexpr int kLin = 23;                    // an edge's record: Jc (12), Jl (6), e_x, e_y, w, rho at the estimate, rho at the trial
constexpr int kCamSums = 27;                // 21 (Hpp, upper triangle by rows) + 6 (bp)
constexpr int kPtSums = 9;                  // 6 (Hll, upper triangle by rows) + 3 (bl)
constexpr int kBlockSums = 42;              // 36 (W Hll^-1 W^T) + 6 (W Hll^-1 bl, diagonal blocks only)

enum Kind : int32_t { kLinearise = 0, kTrial = 1, kClassify = 2, kSolve = 3, kDone = 4 };

// where a job's items sit in the chunk's tables; every index stored in a table is chunk-wide
struct JobRec {
    int32_t cam0, n_cam, pt0, n_pt, e0, n_e, blk0, n_blk, n_free, stage0;
    int64_t s0;                             // of the job's reduced matrix, in doubles
    double fx, fy, cx, cy;
};
struct DevOpt {
    int32_t rounds, iterations[kMaxRounds], robust_rounds, keep_stages, eval;   // eval: one linearisation at the given lambda, nothing else
    float chi2_threshold;
    double delta, lambda;
};
// a job's sequencer state (B8, B9) and what it reports
struct Ctl {
    pose::Lm lm;
    int32_t kind, round, propose, fail, nbad, nflag, n_part, accept, stage, big, pad0, pad1;
    double scale, chi;                      // the last propose's scale, the last reduced chi2
    double r_chi2[kMaxRounds];
    int32_t r_bad[kMaxRounds], r_its[kMaxRounds], r_trials[kMaxRounds];
    int32_t rounds_run, pad2;
};

struct Tab {
    const JobRec* job; Ctl* ctl;
    // cameras
    double* T; double* Tn; const uint8_t* fixed; const int32_t* cjob; const int32_t* cam_off; const int32_t* cam_edges;
    double* cam_sums; int32_t* cam_cnt; int32_t* rank; double* bs; double* dp;
    // points
    double* X; double* Xn; const int32_t* pjob; const int32_t* pt_off; const int32_t* pt_edges;
    double* pt_sums; double* pt_inv; double* pt_chi; double* dl; int32_t* pt_cnt;
    // edges
    const int32_t* ep; const int32_t* ec; const int32_t* ejob; const float* obs; const float* w;
    uint8_t* active; uint8_t* outlier; float* chi2f; double* lin; double* chi2d;
    // blocks of the reduced system (a <= b, both free) and their items
    const int32_t* blk_a; const int32_t* blk_b; const int32_t* blk_job; const int32_t* blk_off; const int32_t* it_p; const int32_t* it_ea; const int32_t* it_eb;
    double* S;
    double* stT; double* stX;               // keep_stages: rounds x (cameras, points) per job
    int32_t* running;
};

IBA_POSE_HD void count(int32_t* p, int32_t v) {
#if defined(__HIP_DEVICE_COMPILE__)
    atomicAdd(p, v);
#else
    *p += v;
#endif
}
IBA_POSE_HD void raise(int32_t* p) {
#if defined(__HIP_DEVICE_COMPILE__)
    atomicOr(p, 1);
#else
    *p = 1;
#endif
}

// ---- B1: the 2 x 3 point Jacobian of EdgeSE3ProjectXYZ::linearizeOplus at p = R X + t (P1's p, the same expressions) ----
IBA_POSE_HD void camera_point(const double* T, double X, double Y, double Z, double* p) {
    p[0] = ((T[0] * X + T[1] * Y) + T[2] * Z) + T[3];
    p[1] = ((T[4] * X + T[5] * Y) + T[6] * Z) + T[7];
    p[2] = ((T[8] * X + T[9] * Y) + T[10] * Z) + T[11];
}
IBA_POSE_HD void point_jacobian(const double* T, const pose::Cam& K, const double* p, double* Jl) {
    const double iz = 1.0 / p[2];
    const double a = (-(K.fx * p[0])) * iz, b = (-(K.fy * p[1])) * iz;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        Jl[c] = (-iz) * (K.fx * T[c] + a * T[8 + c]);
        Jl[3 + c] = (-iz) * (K.fy * T[4 + c] + b * T[8 + c]);
    }
}

// ---- B1, B2, B9: one edge of the chunk, by the kind of its job's next evaluation ----
IBA_POSE_HD void edge_item(const Tab& t, int e, const DevOpt& o) {
    const int j = t.ejob[e];
    Ctl& c = t.ctl[j];
    const int kind = c.kind;
    if (kind == kSolve || kind == kDone) return;
    const JobRec& q = t.job[j];
    const pose::Cam K{q.fx, q.fy, q.cx, q.cy};
    const int cam = t.ec[e], pt = t.ep[e];
    const bool trial = kind == kTrial;
    const double* T = (trial ? t.Tn : t.T) + 12 * (size_t)cam;
    const double* X = (trial ? t.Xn : t.X) + 3 * (size_t)pt;
    const double ox = t.obs[2 * (size_t)e], oy = t.obs[2 * (size_t)e + 1], w = t.w[e];
    double* L = t.lin + (size_t)kLin * e;
    double ex, ey, chi2, rho0, rho1;
    if (kind == kClassify) {
        double p[3];
        camera_point(T, X[0], X[1], X[2], p);
        pose::edge(T, K, X[0], X[1], X[2], ox, oy, w, &ex, &ey, &chi2, nullptr);
        const int bad = (pose::is_outlier(chi2, o.chi2_threshold) || !(p[2] > 0.0)) ? 1 : 0;
        if (c.round == o.rounds - 1) {
            t.outlier[e] = (uint8_t)bad; t.chi2f[e] = pose::canonf((float)chi2);
            if (bad) count(&c.nflag, 1);
        } else if (t.active[e] && bad) {
            t.active[e] = 0;
            count(&c.nbad, 1);
        }
        return;
    }
    const int robust = (o.eval ? o.robust_rounds > 0 : c.round < o.robust_rounds) ? 1 : 0;
    if (trial) {
        if (!t.active[e]) return;
        pose::edge(T, K, X[0], X[1], X[2], ox, oy, w, &ex, &ey, &chi2, nullptr);
        pose::huber(chi2, robust, o.delta, &rho0, &rho1);
        L[22] = rho0;
        return;
    }
    if (!t.active[e] && !t.chi2d) return;
    double p[3];
    camera_point(T, X[0], X[1], X[2], p);
    pose::edge(T, K, X[0], X[1], X[2], ox, oy, w, &ex, &ey, &chi2, L);
    if (t.chi2d) t.chi2d[e] = pose::canon(chi2);
    if (!t.active[e]) return;
    point_jacobian(T, K, p, L + 12);
    pose::huber(chi2, robust, o.delta, &rho0, &rho1);
    L[18] = ex; L[19] = ey; L[20] = rho1 * w; L[21] = rho0;
}

// ---- B3: a point's sums, sequential over its active edges in ascending edge index ----
IBA_POSE_HD void point_item(const Tab& t, int p) {
    const int kind = t.ctl[t.pjob[p]].kind;
    if (kind != kLinearise && kind != kTrial) return;
    double acc[kPtSums], chi = 0.0;
#pragma unroll
    for (int k = 0; k < kPtSums; ++k) acc[k] = 0.0;
    int n = 0;
    for (int k = t.pt_off[p]; k < t.pt_off[p + 1]; ++k) {
        const int e = t.pt_edges[k];
        if (!t.active[e]) continue;
        const double* L = t.lin + (size_t)kLin * e;
        ++n;
        if (kind == kTrial) { chi = chi + L[22]; continue; }
        const double wr = L[20], ex = L[18], ey = L[19];
        const double* J = L + 12;
        int at = 0;
#pragma unroll
        for (int a = 0; a < 3; ++a) {
#pragma unroll
            for (int b = a; b < 3; ++b) { acc[at] = acc[at] + wr * (J[a] * J[b] + J[3 + a] * J[3 + b]); ++at; }
        }
#pragma unroll
        for (int a = 0; a < 3; ++a) acc[6 + a] = acc[6 + a] - wr * (J[a] * ex + J[3 + a] * ey);
        chi = chi + L[21];
    }
    t.pt_chi[p] = chi;
    if (kind == kTrial) return;
    t.pt_cnt[p] = n;
    for (int k = 0; k < kPtSums; ++k) t.pt_sums[(size_t)kPtSums * p + k] = acc[k];
}

// ---- B3: one lane of a free camera's wave: the k-th edge of its list belongs to lane k mod 64; returns the lane's active edges ----
IBA_POSE_HD int camera_lane(const Tab& t, int cam, int lane, double* acc) {
#pragma unroll
    for (int k = 0; k < kCamSums; ++k) acc[k] = 0.0;
    int n = 0;
    for (int k = t.cam_off[cam] + lane; k < t.cam_off[cam + 1]; k += kWave) {
        const int e = t.cam_edges[k];
        if (!t.active[e]) continue;
        const double* L = t.lin + (size_t)kLin * e;
        const double wr = L[20], ex = L[18], ey = L[19];
        ++n;
        int at = 0;
#pragma unroll
        for (int a = 0; a < 6; ++a) {
#pragma unroll
            for (int b = a; b < 6; ++b) { acc[at] = acc[at] + wr * (L[a] * L[b] + L[6 + a] * L[6 + b]); ++at; }
        }
#pragma unroll
        for (int a = 0; a < 6; ++a) acc[21 + a] = acc[21 + a] - wr * (L[a] * ex + L[6 + a] * ey);
    }
    return n;
}
IBA_POSE_HD bool camera_runs(const Tab& t, int cam) { return !t.fixed[cam] && t.ctl[t.cjob[cam]].kind == kLinearise; }

// ---- B3, B8: one lane of a job's chi2 (point p on lane p mod 256) and of its largest diagonal ----
IBA_POSE_HD double chi_lane(const Tab& t, const JobRec& q, int lane) {
    double s = 0.0;
    for (int p = q.pt0 + lane; p < q.pt0 + q.n_pt; p += kLanes) if (t.pt_cnt[p] > 0) s = s + t.pt_chi[p];
    return s;
}
IBA_POSE_HD double larger(double a, double b) { return b > a ? b : a; }
IBA_POSE_HD double diag_lane(const Tab& t, const JobRec& q, int lane) {
    double m = 0.0;
    for (int p = q.pt0 + lane; p < q.pt0 + q.n_pt; p += kLanes) {
        if (t.pt_cnt[p] <= 0) continue;
        const double* h = t.pt_sums + (size_t)kPtSums * p;
        m = larger(m, std::fabs(h[0])); m = larger(m, std::fabs(h[3])); m = larger(m, std::fabs(h[5]));
    }
    for (int c = q.cam0 + lane; c < q.cam0 + q.n_cam; c += kLanes) {
        if (t.fixed[c] || t.cam_cnt[c] <= 0) continue;
        for (int k = 0; k < 6; ++k) m = larger(m, std::fabs(t.cam_sums[(size_t)kCamSums * c + pose::hidx(k, k)]));
    }
    return m;
}

// the end of an LM iteration: what the job evaluates next
IBA_POSE_HD void iteration_over(Ctl& c, const DevOpt& o) {
    ++c.lm.it;
    c.kind = (c.lm.stop || c.lm.it >= o.iterations[c.round]) ? kClassify : kLinearise;
    c.propose = 0;
}

// ---- B8, B9: the sequencer's first half, one lane per job after an evaluation's sums: chi = the job's reduced chi2, md = its largest diagonal ----
IBA_POSE_HD void sequence_front(const Tab& t, int j, const DevOpt& o, double chi, double md) {
    Ctl& c = t.ctl[j];
    const JobRec& q = t.job[j];
    c.accept = 0; c.stage = -1; c.fail = 0; c.chi = chi;
    switch (c.kind) {
    case kLinearise: {
        c.lm.current = chi;
        if (o.eval) c.lm.lambda = o.lambda;
        else if (c.lm.it == 0) { c.lm.lambda = 1e-5 * md; c.lm.ni = 2.0; }
        c.lm.qmax = 0; c.lm.rho = 0.0; c.lm.stop = 0; c.lm.again = 0;
        ++c.lm.its;
        int r = 0;                                            // B4: the rows of the reduced system
        for (int cam = q.cam0; cam < q.cam0 + q.n_cam; ++cam) t.rank[cam] = (!t.fixed[cam] && t.cam_cnt[cam] > 0) ? r++ : -1;
        c.n_part = r;
        c.propose = 1;
        break;
    }
    case kTrial:
        if (pose::lm_verdict(&c.lm, 1, c.scale, chi)) c.accept = 1;   // B8: P5's verdict, the scale over all participating unknowns
        if (c.lm.again) c.propose = 1; else iteration_over(c, o);
        break;
    case kSolve:
        c.propose = 1;
        break;
    case kClassify: {
        const int r = c.round;
        c.r_chi2[r] = pose::canon(c.lm.current); c.r_bad[r] = (r == o.rounds - 1) ? c.nflag : c.nbad; c.r_its[r] = c.lm.its; c.r_trials[r] = c.lm.trials;
        c.rounds_run = r + 1;
        if (o.keep_stages) c.stage = r;
        c.round = r + 1;
        c.propose = 0;
        if (c.round < o.rounds) { c.kind = kLinearise; pose::lm_round_start(&c.lm); } else c.kind = kDone;
        break;
    }
    default:
        c.propose = 0;
        break;
    }
}
// what the lanes of a job copy after sequence_front: an accepted trial into the estimate, the estimate into a kept stage
IBA_POSE_HD void copy_item(const Tab& t, int j, int i, int stride) {
    const Ctl& c = t.ctl[j];
    const JobRec& q = t.job[j];
    const int nT = 12 * q.n_cam, nX = 3 * q.n_pt;
    if (c.accept) {
        for (int k = i; k < nT; k += stride) t.T[12 * (size_t)q.cam0 + k] = t.Tn[12 * (size_t)q.cam0 + k];
        for (int k = i; k < nX; k += stride) t.X[3 * (size_t)q.pt0 + k] = t.Xn[3 * (size_t)q.pt0 + k];
    }
    if (c.stage >= 0) {
        double* sT = t.stT + (size_t)kMaxRounds * 12 * q.cam0 + (size_t)c.stage * nT;
        double* sX = t.stX + (size_t)kMaxRounds * 3 * q.pt0 + (size_t)c.stage * nX;
        for (int k = i; k < nT; k += stride) sT[k] = t.T[12 * (size_t)q.cam0 + k];
        for (int k = i; k < nX; k += stride) sX[k] = t.X[3 * (size_t)q.pt0 + k];
    }
}

// ---- B5: (Hll + lambda I)^-1 of a participating point by cofactors; a determinant that is not positive and finite fails the trial ----
IBA_POSE_HD void inverse_item(const Tab& t, int p) {
    Ctl& c = t.ctl[t.pjob[p]];
    if (!c.propose || t.pt_cnt[p] <= 0) return;
    const double* h = t.pt_sums + (size_t)kPtSums * p;
    const double l = c.lm.lambda;
    const double a00 = h[0] + l, a01 = h[1], a02 = h[2], a11 = h[3] + l, a12 = h[4], a22 = h[5] + l;
    const double c00 = a11 * a22 - a12 * a12, c01 = a02 * a12 - a01 * a22, c02 = a01 * a12 - a02 * a11;
    const double c11 = a00 * a22 - a02 * a02, c12 = a01 * a02 - a00 * a12, c22 = a00 * a11 - a01 * a01;
    const double det = (a00 * c00 + a01 * c01) + a02 * c02;
    if (!(det > 0.0) || !(det <= pose::kMax)) { raise(&c.fail); return; }
    const double id = 1.0 / det;
    double* v = t.pt_inv + 6 * (size_t)p;
    v[0] = c00 * id; v[1] = c01 * id; v[2] = c02 * id; v[3] = c11 * id; v[4] = c12 * id; v[5] = c22 * id;
}
// W = w Jc^T Jl (6 x 3) of an edge's record
IBA_POSE_HD void edge_w(const double* L, double* W) {
    const double wr = L[20];
#pragma unroll
    for (int r = 0; r < 6; ++r) {
#pragma unroll
        for (int c = 0; c < 3; ++c) W[3 * r + c] = wr * (L[r] * L[12 + c] + L[6 + r] * L[15 + c]);
    }
}
IBA_POSE_HD double sym3(const double* v, int r, int c) { return v[r <= c ? (r == 0 ? c : r + c + 1) : (c == 0 ? r : r + c + 1)]; }

// ---- B6: one lane of a block's wave: the k-th item of the block's list belongs to lane k mod 64; an item with an inactive edge is skipped ----
IBA_POSE_HD bool block_runs(const Tab& t, int blk) {
    const Ctl& c = t.ctl[t.blk_job[blk]];
    return c.propose && !c.fail && t.rank[t.blk_a[blk]] >= 0 && t.rank[t.blk_b[blk]] >= 0;
}
IBA_POSE_HD void block_lane(const Tab& t, int blk, int lane, double* acc) {
#pragma unroll
    for (int k = 0; k < kBlockSums; ++k) acc[k] = 0.0;
    const bool diag = t.blk_a[blk] == t.blk_b[blk];
    for (int k = t.blk_off[blk] + lane; k < t.blk_off[blk + 1]; k += kWave) {
        const int ea = t.it_ea[k], eb = t.it_eb[k], p = t.it_p[k];
        if (!t.active[ea] || !t.active[eb]) continue;
        const double* hi = t.pt_inv + 6 * (size_t)p;
        double Wa[18], Wb[18], Y[18];
        edge_w(t.lin + (size_t)kLin * ea, Wa);
        edge_w(t.lin + (size_t)kLin * eb, Wb);
#pragma unroll
        for (int r = 0; r < 6; ++r) {
#pragma unroll
            for (int c = 0; c < 3; ++c) Y[3 * r + c] = (Wa[3 * r] * sym3(hi, 0, c) + Wa[3 * r + 1] * sym3(hi, 1, c)) + Wa[3 * r + 2] * sym3(hi, 2, c);
        }
#pragma unroll
        for (int r = 0; r < 6; ++r) {
#pragma unroll
            for (int s = 0; s < 6; ++s) acc[6 * r + s] = acc[6 * r + s] + ((Y[3 * r] * Wb[3 * s] + Y[3 * r + 1] * Wb[3 * s + 1]) + Y[3 * r + 2] * Wb[3 * s + 2]);
        }
        if (diag) {
            const double* bl = t.pt_sums + (size_t)kPtSums * p + 6;
#pragma unroll
            for (int r = 0; r < 6; ++r) acc[36 + r] = acc[36 + r] + ((Y[3 * r] * bl[0] + Y[3 * r + 1] * bl[1]) + Y[3 * r + 2] * bl[2]);
        }
    }
}
// the reduced matrix is kept as its lower triangle, entry (i, k), i >= k, at S[k n + i]
IBA_POSE_HD size_t sidx(int n, int i, int k) { return (size_t)k * n + i; }
IBA_POSE_HD void block_store(const Tab& t, int blk, const double* sum) {
    const int j = t.blk_job[blk], a = t.blk_a[blk], b = t.blk_b[blk];
    const Ctl& c = t.ctl[j];
    const JobRec& q = t.job[j];
    const int n = 6 * c.n_part, ra = 6 * t.rank[a], rb = 6 * t.rank[b];
    double* S = t.S + q.s0;
    if (a == b) {
        const double* h = t.cam_sums + (size_t)kCamSums * a;
        for (int r = 0; r < 6; ++r) {
            for (int s = 0; s <= r; ++s) S[sidx(n, ra + r, ra + s)] = (h[pose::hidx(s, r)] + (r == s ? c.lm.lambda : 0.0)) - sum[6 * r + s];
            t.bs[6 * (size_t)a + r] = h[21 + r] - sum[36 + r];
        }
    } else {
        for (int r = 0; r < 6; ++r) for (int s = 0; s < 6; ++s) S[sidx(n, rb + s, ra + r)] = -sum[6 * r + s];
    }
}

// ---- B7: the reduced solve, entry by entry: Cholesky without pivoting, the forward and the backward substitution. The kernel's parallel form gives
// the same bytes: every entry is its a_ij with the products subtracted one at a time in the stated order. false: a pivot not positive and finite. ----
IBA_POSE_HD bool pivot_ok(double s) { return s > 0.0 && s <= pose::kMax; }
inline bool reduced_solve(double* S, int n, const double* b, double* x, double* y) {
    for (int j = 0; j < n; ++j) {
        double s = S[sidx(n, j, j)];
        for (int k = 0; k < j; ++k) s = s - S[sidx(n, j, k)] * S[sidx(n, j, k)];
        if (!pivot_ok(s)) return false;
        const double ljj = std::sqrt(s);
        S[sidx(n, j, j)] = ljj;
        for (int i = j + 1; i < n; ++i) {
            double v = S[sidx(n, i, j)];
            for (int k = 0; k < j; ++k) v = v - S[sidx(n, i, k)] * S[sidx(n, j, k)];
            S[sidx(n, i, j)] = v / ljj;
        }
    }
    for (int i = 0; i < n; ++i) { double v = b[i]; for (int k = 0; k < i; ++k) v = v - S[sidx(n, i, k)] * y[k]; y[i] = v / S[sidx(n, i, i)]; }
    for (int i = n - 1; i >= 0; --i) { double v = y[i]; for (int k = n - 1; k > i; --k) v = v - S[sidx(n, k, i)] * x[k]; x[i] = v / S[sidx(n, i, i)]; }
    return true;
}

// ---- B7: a point's step dl = (Hll + lambda I)^-1 (bl - sum_a W_pa^T dp_a), its edges ascending, and its trial position ----
IBA_POSE_HD void backsub_item(const Tab& t, int p) {
    const Ctl& c = t.ctl[t.pjob[p]];
    if (!c.propose || c.fail) return;
    const double* X = t.X + 3 * (size_t)p;
    double* Xn = t.Xn + 3 * (size_t)p;
    double* dl = t.dl + 3 * (size_t)p;
    if (t.pt_cnt[p] <= 0) { for (int k = 0; k < 3; ++k) { Xn[k] = X[k]; dl[k] = 0.0; } return; }
    const double* h = t.pt_sums + (size_t)kPtSums * p;
    double v[3] = {h[6], h[7], h[8]};
    for (int k = t.pt_off[p]; k < t.pt_off[p + 1]; ++k) {
        const int e = t.pt_edges[k];
        if (!t.active[e]) continue;
        const int cam = t.ec[e];
        if (t.rank[cam] < 0) continue;
        const double* d = t.dp + 6 * (size_t)cam;
        double W[18];
        edge_w(t.lin + (size_t)kLin * e, W);
#pragma unroll
        for (int a = 0; a < 3; ++a) v[a] = v[a] - (((((W[a] * d[0] + W[3 + a] * d[1]) + W[6 + a] * d[2]) + W[9 + a] * d[3]) + W[12 + a] * d[4]) + W[15 + a] * d[5]);
    }
    const double* hi = t.pt_inv + 6 * (size_t)p;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        dl[a] = (sym3(hi, a, 0) * v[0] + sym3(hi, a, 1) * v[1]) + sym3(hi, a, 2) * v[2];
        Xn[a] = X[a] + dl[a];
    }
}
// a camera's trial pose: P6 for a camera with a row, its pose otherwise
IBA_POSE_HD void camera_update_item(const Tab& t, int cam) {
    Ctl& c = t.ctl[t.cjob[cam]];
    if (!c.propose || c.fail) return;
    const double* T = t.T + 12 * (size_t)cam;
    double* Tn = t.Tn + 12 * (size_t)cam;
    if (t.rank[cam] < 0) { for (int k = 0; k < 12; ++k) Tn[k] = T[k]; return; }
    if (pose::exp_update(t.dp + 6 * (size_t)cam, T, Tn)) count(&c.big, 1);
}

// ---- B8: the sequencer's second half, one lane per job after a propose: the scale, or the verdict on a failed factorisation ----
IBA_POSE_HD void sequence_back(const Tab& t, int j, const DevOpt& o) {
    Ctl& c = t.ctl[j];
    const JobRec& q = t.job[j];
    if (c.propose) {
        ++c.lm.trials;
        if (!c.fail) {
            double scale = 1e-3;
            const double l = c.lm.lambda;
            for (int cam = q.cam0; cam < q.cam0 + q.n_cam; ++cam) {
                if (t.rank[cam] < 0) continue;
                const double* d = t.dp + 6 * (size_t)cam;
                const double* b = t.cam_sums + (size_t)kCamSums * cam + 21;
                for (int k = 0; k < 6; ++k) scale = scale + d[k] * (l * d[k] + b[k]);
            }
            for (int p = q.pt0; p < q.pt0 + q.n_pt; ++p) {
                if (t.pt_cnt[p] <= 0) continue;
                const double* d = t.dl + 3 * (size_t)p;
                const double* b = t.pt_sums + (size_t)kPtSums * p + 6;
                for (int k = 0; k < 3; ++k) scale = scale + d[k] * (l * d[k] + b[k]);
            }
            c.scale = scale;
            c.kind = o.eval ? kDone : kTrial;
        } else if (o.eval) {
            c.kind = kDone;
        } else {
            pose::lm_verdict(&c.lm, 0, 0.0, 0.0);
            if (c.lm.again) c.kind = kSolve; else iteration_over(c, o);
        }
        c.propose = 0;
    }
    if (c.kind != kDone) count(t.running, 1);
}

}  // namespace bundle
}  // namespace iba
