"""Numpy restatement of the pose-graph optimiser's rules (include/iba_mi355x.h, iba_pgo_*; rule numbers as there): test infrastructure.
  * linearize(..., dtype=np.float64): rules 2-5 over all edges at once, every expression in the order the header gives (and the device uses); with
    dtype=np.longdouble the same rules with atan2 / sqrt / sin / cos in long double: the yardstick the parity gates measure both sides against.
  * dense_system / dense_solve: H as a dense 6N x 6N and numpy.linalg.solve — what Open3D does per LM trial.
  * sparse_system / sparse_solve: the same H in scipy.sparse and its direct solve, for the sizes the dense H cannot follow to; block_residual: the
    figure of the solve gate in long double from H's 6x6 blocks, without H.
  * plan: the arrowhead plan (chain / cross edges, separators, K doubling, runs) as plain Python.
  * optimize: rules 6 and 7; records every rho and every stopping comparison, check_margins asserts that none is a near-tie.
  * make_graph: the seeded generator (smooth trajectory, noisy odometry, loop edges, informations of the sum G^T G form of iba_scan_information).
"""
import numpy as np

EPS = 2.220446049250313e-16
STOP_NONE, STOP_RIGHT_TERM, STOP_INCREMENT, STOP_RESIDUAL_INCREMENT, STOP_RESIDUAL, STOP_MAX_ITERATION = 0, 1, 2, 3, 4, 5
MAX_SEPARATORS = 1024

DEFAULTS = dict(max_corr_dist=1.2, edge_prune_threshold=0.25, preference_loop_closure=1.0, reference_node=0, max_iteration=100, max_iteration_lm=20,
                min_relative_increment=1e-6, min_relative_residual_increment=1e-6, min_right_term=1e-6, min_residual=1e-6,
                upper_scale_factor=2.0 / 3.0, lower_scale_factor=1.0 / 3.0, segment=128)


def options(**kw):
    o = dict(DEFAULTS)
    for k in kw:
        if k not in o:
            raise KeyError(k)
    o.update(kw)
    return o


# ---- rigid 3x4 algebra on stacks [n, 3, 4] (a [n, 4, 4] stack works too: the last row is never read) ----
def mul12(A, B):
    C = np.empty(A.shape[:1] + (3, 4), A.dtype)
    for r in range(3):
        for c in range(4):
            v = (A[:, r, 0] * B[:, 0, c] + A[:, r, 1] * B[:, 1, c]) + A[:, r, 2] * B[:, 2, c]
            C[:, r, c] = v + A[:, r, 3] if c == 3 else v
    return C


def inv12(A):
    O = np.empty(A.shape[:1] + (3, 4), A.dtype)
    for r in range(3):
        for c in range(3):
            O[:, r, c] = A[:, c, r]
        O[:, r, 3] = -((A[:, 0, r] * A[:, 0, 3] + A[:, 1, r] * A[:, 1, 3]) + A[:, 2, r] * A[:, 2, 3])
    return O


def to44(A12):
    out = np.zeros(A12.shape[:1] + (4, 4), A12.dtype)
    out[:, :3, :] = A12[:, :3, :]
    out[:, 3, 3] = 1
    return out


def vec6(M):
    """rule 1 on a stack [n, >=3, 4] -> [n, 6]"""
    sy = np.sqrt(M[:, 0, 0] * M[:, 0, 0] + M[:, 1, 0] * M[:, 1, 0])
    big = sy >= 1e-6
    v = np.empty((len(M), 6), M.dtype)
    v[:, 0] = np.where(big, np.arctan2(M[:, 2, 1], M[:, 2, 2]), np.arctan2(-M[:, 1, 2], M[:, 1, 1]))
    v[:, 1] = np.arctan2(-M[:, 2, 0], sy)
    v[:, 2] = np.where(big, np.arctan2(M[:, 1, 0], M[:, 0, 0]), 0)
    v[:, 3:] = M[:, :3, 3]
    return v


def T_of(v):
    """the inverse of rule 1: Rz(c) Ry(b) Rx(a) with the translation, stack [n, 6] -> [n, 4, 4]"""
    v = np.atleast_2d(v)
    ca, sa, cb, sb, cg, sg = np.cos(v[:, 0]), np.sin(v[:, 0]), np.cos(v[:, 1]), np.sin(v[:, 1]), np.cos(v[:, 2]), np.sin(v[:, 2])
    T = np.zeros((len(v), 4, 4), v.dtype)
    T[:, 0, 0] = cg * cb; T[:, 0, 1] = cg * sb * sa - sg * ca; T[:, 0, 2] = cg * sb * ca + sg * sa
    T[:, 1, 0] = sg * cb; T[:, 1, 1] = sg * sb * sa + cg * ca; T[:, 1, 2] = sg * sb * ca - cg * sa
    T[:, 2, 0] = -sb; T[:, 2, 1] = cb * sa; T[:, 2, 2] = cb * ca
    T[:, :3, 3] = v[:, 3:]
    T[:, 3, 3] = 1
    return T


def generators():
    G = np.zeros((6, 4, 4))
    G[0, 1, 2], G[0, 2, 1] = -1, 1
    G[1, 0, 2], G[1, 2, 0] = 1, -1
    G[2, 0, 1], G[2, 1, 0] = -1, 1
    for k in range(3):
        G[3 + k, k, 3] = 1
    return G


def lin6(M):
    return np.array([(M[2, 1] - M[1, 2]) / 2, (M[0, 2] - M[2, 0]) / 2, (M[1, 0] - M[0, 1]) / 2, M[0, 3], M[1, 3], M[2, 3]])


def jacobian_dense(X, Pt, Ps, of_target=False):
    """rule 3 as the text reads, with plain 4x4 products: column k = lin6(X^-1 pose_t^-1 G_k pose_s); of_target: the derivative in the TARGET's
    increment, d/dh (exp(h G_k) pose_t)^-1 = -pose_t^-1 G_k, i.e. Jt"""
    Xi, Ti = np.linalg.inv(X), np.linalg.inv(Pt)
    G = generators()
    J = np.zeros((6, 6))
    for k in range(6):
        J[:, k] = lin6(Xi @ Ti @ (-G[k] if of_target else G[k]) @ Ps)
    return J


class Graph:
    """nodes [N, 4, 4]; src / tgt [E] int; X [E, 4, 4]; info [E, 6, 6] (mirrored from the upper triangle); uncertain [E] bool"""

    def __init__(self, nodes, src, tgt, X, info, uncertain, truth=None):
        self.nodes = np.ascontiguousarray(nodes, np.float64).reshape(-1, 4, 4)
        self.src, self.tgt = np.asarray(src, np.int64).reshape(-1), np.asarray(tgt, np.int64).reshape(-1)
        E = len(self.src)
        self.X = np.ascontiguousarray(X, np.float64).reshape(E, 4, 4)
        info = np.asarray(info, np.float64).reshape(E, 6, 6)
        up = np.triu(np.ones((6, 6), bool))
        self.info = np.where(up, info, np.transpose(info, (0, 2, 1)))
        self.uncertain = np.asarray(uncertain, bool).reshape(E)
        self.truth = truth

    @property
    def N(self):
        return len(self.nodes)

    @property
    def E(self):
        return len(self.src)

    def edge_tuples(self):
        return [(int(self.src[e]), int(self.tgt[e]), self.X[e], self.info[e], bool(self.uncertain[e])) for e in range(self.E)]


def edge_terms(nodes, g, dtype=np.float64, want_js=True):
    """rules 2 and 3 per edge: zeta [E, 6], Js [E, 6, 6], q = zeta^T L zeta [E], Lz [E, 6]"""
    E = g.E
    P = nodes.astype(dtype)
    Xi = inv12(g.X.astype(dtype))
    Ps, Pt = P[g.src], P[g.tgt]
    B = mul12(Xi, inv12(Pt))
    M = mul12(B, Ps)
    zeta = vec6(M)
    L = g.info.astype(dtype)
    Lz = np.empty((E, 6), dtype)
    q = np.zeros(E, dtype)
    for i in range(6):
        s = L[:, i, 0] * zeta[:, 0]
        for j in range(1, 6):
            s = s + L[:, i, j] * zeta[:, j]
        Lz[:, i] = s
        q = zeta[:, 0] * s if i == 0 else q + zeta[:, i] * s
    Js = None
    if want_js:
        Js = np.zeros((E, 6, 6), dtype)
        for k in range(3):
            k1, k2 = (k + 1) % 3, (k + 2) % 3
            Q = np.zeros((E, 3, 4), dtype)
            Q[:, k1] = -Ps[:, k2, :]
            Q[:, k2] = Ps[:, k1, :]
            W = np.empty((E, 3, 4), dtype)
            for r in range(3):
                for c in range(4):
                    W[:, r, c] = (B[:, r, 0] * Q[:, 0, c] + B[:, r, 1] * Q[:, 1, c]) + B[:, r, 2] * Q[:, 2, c]
            Js[:, 0, k] = (W[:, 2, 1] - W[:, 1, 2]) * 0.5
            Js[:, 1, k] = (W[:, 0, 2] - W[:, 2, 0]) * 0.5
            Js[:, 2, k] = (W[:, 1, 0] - W[:, 0, 1]) * 0.5
            Js[:, 3:, k] = W[:, :, 3]
        for k in range(3, 6):
            Js[:, 3:, k] = B[:, :, k - 3]
    return zeta, Js, q, Lz


def line_process_mu(g, opt, pruned):
    sel = g.uncertain & ~pruned
    if not sel.any():
        return 0.0
    s = 0.0
    for e in np.where(sel)[0]:
        s += g.info[e, 5, 5]
    return opt["preference_loop_closure"] * (opt["max_corr_dist"] * opt["max_corr_dist"]) * (s / float(sel.sum()))


def line_weights(g, q, mu, pruned, old):
    den = mu + q
    with np.errstate(divide="ignore", invalid="ignore"):
        w = np.where(den != 0, (mu / np.where(den != 0, den, 1)) ** 2, 1.0)
    w = np.where(g.uncertain, w, 1.0)
    return np.where(pruned, old, w)


def linearize(nodes, g, weight, pruned=None, dtype=np.float64):
    """-> dict(zeta, A [E, 6, 6], g [E, 6], c [E], D [N, 6, 6], b [N, 6], residual, q, terms): sums over a node's edges in ascending edge index;
    `terms` holds, per output, the sum of the absolute values of the terms of its largest sum (the scale two summation orders may differ by)"""
    E, N = g.E, len(nodes)
    pruned = np.zeros(E, bool) if pruned is None else pruned
    zeta, Js, q, Lz = edge_terms(nodes, g, dtype)
    L = g.info.astype(dtype)
    w = np.where(pruned, 0, np.asarray(weight)).astype(dtype)
    LJ = np.empty((E, 6, 6), dtype)
    for i in range(6):
        for k in range(6):
            a = L[:, i, 0] * Js[:, 0, k]
            for j in range(1, 6):
                a = a + L[:, i, j] * Js[:, j, k]
            LJ[:, i, k] = a
    A = np.empty((E, 6, 6), dtype)
    Aabs = np.zeros((E, 6, 6), dtype)
    for k in range(6):
        for l in range(k, 6):
            a = Js[:, 0, k] * LJ[:, 0, l]
            t = np.abs(a)
            for i in range(1, 6):
                a = a + Js[:, i, k] * LJ[:, i, l]
                t = t + np.abs(Js[:, i, k] * LJ[:, i, l])
            A[:, k, l] = w * a
            A[:, l, k] = A[:, k, l]
            Aabs[:, k, l] = Aabs[:, l, k] = w * t
    gv = np.empty((E, 6), dtype)
    for k in range(6):
        a = Js[:, 0, k] * Lz[:, 0]
        for i in range(1, 6):
            a = a + Js[:, i, k] * Lz[:, i]
        gv[:, k] = w * a
    c = w * q
    D = np.zeros((N, 6, 6), dtype)
    b = np.zeros((N, 6), dtype)
    babs = np.zeros((N, 6), dtype)
    for e in range(E):
        if pruned[e]:
            continue
        s, t = g.src[e], g.tgt[e]
        D[s] += A[e]; D[t] += A[e]
        b[s] += -gv[e]; b[t] += gv[e]
        babs[s] += np.abs(gv[e]); babs[t] += np.abs(gv[e])
    residual = dtype(0)
    for e in range(E):
        residual = residual + c[e]
    terms = dict(zeta=float(np.max(np.abs(zeta))) if E else 0.0, A=float(np.max(Aabs)) if E else 0.0, b=float(np.max(babs)) if E else 0.0,
                 residual=float(np.sum(np.abs(c))) if E else 0.0, weight=1.0)
    return dict(zeta=zeta, A=A, g=gv, c=c, D=D, b=b, residual=residual, q=q, terms=terms)


def dense_system(N, g, A, b, pruned=None):
    """H [6N, 6N] from the edge blocks (H_ss += A, H_tt += A, H_st = H_ts -= A) and the stacked b"""
    H = np.zeros((6 * N, 6 * N))
    for e in range(g.E):
        if pruned is not None and pruned[e]:
            continue
        s, t = 6 * int(g.src[e]), 6 * int(g.tgt[e])
        H[s:s + 6, s:s + 6] += A[e]; H[t:t + 6, t:t + 6] += A[e]
        H[s:s + 6, t:t + 6] -= A[e]; H[t:t + 6, s:s + 6] -= A[e]
    return H, np.asarray(b, np.float64).reshape(-1)


def dense_solve(H, b, lam):
    return np.linalg.solve(H + lam * np.eye(len(H)), b)


def system_blocks(N, pairs, A):
    """the 6x6 blocks of H, each summed on its own in float64 in the order of `pairs` = (row node, column node, sign, index into A): what the dense
    += / -= of dense_system does to the same entries -> (keys [nb, 2], blocks [nb, 6, 6])"""
    blocks = {}
    for i, j, sign, e in pairs:
        blk = blocks.get((i, j))
        if blk is None:
            blk = blocks[(i, j)] = np.zeros((6, 6))
        if sign > 0:
            blk += A[e]
        else:
            blk -= A[e]
    return np.array(list(blocks.keys()), np.int64).reshape(-1, 2), np.stack(list(blocks.values())) if blocks else np.zeros((0, 6, 6))


def blocks_to_csc(N, keys, vals):
    import scipy.sparse as sp
    k6 = np.arange(6)
    rows = (6 * keys[:, 0])[:, None, None] + k6[None, :, None] + 0 * k6[None, None, :]
    cols = (6 * keys[:, 1])[:, None, None] + 0 * k6[None, :, None] + k6[None, None, :]
    return sp.coo_matrix((vals.reshape(-1), (rows.reshape(-1), cols.reshape(-1))), shape=(6 * N, 6 * N)).tocsc()


def blocks_residual(N, keys, vals, b, lam, delta):
    """|(H + lam I) delta - b| / |b| in long double from the blocks of H; without a right-hand side the plain norm"""
    bl, dl = np.asarray(b, np.longdouble).reshape(N, 6), np.asarray(delta, np.longdouble).reshape(N, 6)
    r = np.longdouble(lam) * dl - bl
    V, x = vals.astype(np.longdouble), dl[keys[:, 1]]
    y = np.zeros((len(keys), 6), np.longdouble)
    for k in range(6):
        y = y + V[:, :, k] * x[:, k:k + 1]
    np.add.at(r, keys[:, 0], y)
    nb = float(np.sqrt(np.sum(bl * bl)))
    return float(np.sqrt(np.sum(r * r))) / nb if nb > 0 else float(np.sqrt(np.sum(r * r)))


def _edge_pairs(g, pruned):
    for e in range(g.E):
        if pruned is not None and pruned[e]:
            continue
        s, t = int(g.src[e]), int(g.tgt[e])
        yield s, s, 1.0, e
        yield t, t, 1.0, e
        yield s, t, -1.0, e
        yield t, s, -1.0, e


def sparse_system(N, g, A, pruned=None):
    """the H of dense_system as a scipy.sparse CSC matrix, entry for entry (at N = 4541 the dense H would take 5.9 GB)"""
    return blocks_to_csc(N, *system_blocks(N, _edge_pairs(g, pruned), A))


def sparse_solve(H, b, lam):
    import scipy.sparse as sp
    import scipy.sparse.linalg as spl
    return spl.spsolve((H + lam * sp.identity(H.shape[0], format="csc")).tocsc(), np.asarray(b, np.float64).reshape(-1))


def block_residual(N, g, A, b, lam, delta, pruned=None):
    """|(H + lam I) delta - b| / |b| in long double without forming H: the figure _rel_residual of the device tests takes from the dense H. The
    blocks are H's own, float64 sums of the A_e: a solve's residual sits at the rounding level of those sums (1e-16 |b|), so applying every A_e
    on its own, as exact arithmetic would allow (y = A_e (delta_s - delta_t), r_s += y, r_t -= y), gives another figure there — on SOLVE_CASES' n3
    1.15e-16 against 9.2e-17 — while on H's blocks the two agree to the order of a long-double sum."""
    return blocks_residual(N, *system_blocks(N, _edge_pairs(g, pruned), np.asarray(A, np.float64).reshape(-1, 6, 6)), b, lam, delta)


def plan(N, src, tgt, segment, cap=MAX_SEPARATORS, active=None):
    """-> dict(separators, runs [(first, last)], K, chain [N]); ValueError when the separators cannot be brought under cap"""
    chain = [-1] * N
    endpoint = [False] * N
    for e, (s, t) in enumerate(zip(src, tgt)):
        if active is not None and not active[e]:
            continue
        lo, hi = (int(s), int(t)) if s < t else (int(t), int(s))
        if hi == lo + 1 and chain[lo] < 0:
            chain[lo] = e
            continue
        endpoint[lo] = endpoint[hi] = True
    n_end = sum(endpoint)
    if n_end > cap:
        raise ValueError("the cross edges touch %d nodes, beyond the separator cap %d" % (n_end, cap))
    K = int(segment)
    while True:
        sep = [i for i in range(N) if endpoint[i] or i % K == 0]
        if len(sep) <= cap:
            break
        if K >= N:
            raise ValueError("the cross edges touch %d nodes: with node 0 that is beyond the separator cap %d" % (n_end, cap))
        K *= 2
    is_sep = set(sep)
    runs = []
    for i in range(N):
        if i in is_sep:
            continue
        if runs and runs[-1][1] == i - 1:
            runs[-1][1] = i
        else:
            runs.append([i, i])
    return dict(separators=sep, runs=[tuple(r) for r in runs], K=K, chain=chain)


def apply_delta(nodes, delta):
    return to44(mul12(T_of(np.asarray(delta).reshape(-1, 6)), nodes))


def lm_pass(nodes, g, opt, pruned, ld=False, log=None):
    """rule 6 -> (nodes, weight, dict(iterations, trials, stop, residual, lam, trace)). ld: linearise in long double and round (the twin)."""
    dt = np.longdouble if ld else np.float64
    N = len(nodes)
    log = log if log is not None else dict(rho=[], cmp=[])
    mu = line_process_mu(g, opt, pruned)
    weight = np.where(pruned, np.nan, 1.0)

    def lin(nd, w):
        r = linearize(nd, g, w, pruned, dt)
        H, b = dense_system(N, g, r["A"].astype(np.float64), r["b"].astype(np.float64), pruned)
        return H, b, float(r["residual"]), r["q"].astype(np.float64)

    def cmp(kind, lhs, rhs):
        log["cmp"].append((kind, float(lhs), float(rhs)))
        return lhs < rhs

    ref_before = nodes[opt["reference_node"]].copy() if opt["reference_node"] >= 0 else None
    H, b, r, _ = lin(nodes, weight)
    lam, nu = 1e-5 * (float(np.max(np.diag(H))) if H.size else 0.0), 2.0
    stop, iterations, trials, trace = STOP_NONE, 0, 0, []
    while stop == STOP_NONE:
        if cmp("right_term", float(np.max(np.abs(b))) if b.size else 0.0, opt["min_right_term"]):
            stop = STOP_RIGHT_TERM
            break
        if iterations >= opt["max_iteration"]:
            stop = STOP_MAX_ITERATION
            break
        x = vec6(nodes).reshape(-1)
        xnorm = float(np.sqrt(np.sum(x * x)))
        for _ in range(opt["max_iteration_lm"]):
            delta = dense_solve(H, b, lam)
            trials += 1
            if cmp("increment", float(np.sqrt(np.sum(delta * delta))), opt["min_relative_increment"] * (xnorm + opt["min_relative_increment"])):
                stop = STOP_INCREMENT
                trace.append(2)
                break
            trial = apply_delta(nodes, delta)
            zeta, _, q, _ = edge_terms(trial, g, dt, want_js=False)
            cs = (np.where(pruned, 0.0, weight).astype(dt) * q).astype(dt)
            acc = dt(0)
            for e in range(g.E):
                acc = acc + cs[e]
            r_new = float(acc)
            rho = (r - r_new) / (float(delta @ (lam * delta + b)) + 1e-3)
            log["rho"].append(rho)
            if rho > 0:
                t = 2.0 * rho - 1.0
                lam *= max(opt["lower_scale_factor"], min(1.0 - t * t * t, opt["upper_scale_factor"]))
                nu = 2.0
                trace.append(1)
                nodes = trial
                r_before = r
                weight = line_weights(g, q.astype(np.float64), mu, pruned, weight)
                H, b, r, _ = lin(nodes, weight)
                if cmp("residual_increment", r_before - r_new, opt["min_relative_residual_increment"] * r_before):
                    stop = STOP_RESIDUAL_INCREMENT
                break
            trace.append(0)
            lam *= nu
            nu *= 2.0
        iterations += 1
        if stop == STOP_NONE and cmp("residual", r, opt["min_residual"]):
            stop = STOP_RESIDUAL
    if ref_before is not None:
        C = mul12(ref_before[None], inv12(nodes[opt["reference_node"]][None]))
        nodes = to44(mul12(np.repeat(C, N, axis=0), nodes))
    return nodes, weight, dict(iterations=iterations, trials=trials, stop=stop, residual=r, lam=lam, trace=trace)


def optimize(g, opt, ld=False):
    """rules 6 and 7 -> dict(nodes, weight, pruned, passes [2], n_pruned, log)"""
    log = dict(rho=[], cmp=[])
    pruned = np.zeros(g.E, bool)
    nodes, w1, p1 = lm_pass(g.nodes.copy(), g, opt, pruned, ld, log)
    drop = g.uncertain & (w1 < opt["edge_prune_threshold"])
    for e in np.where(g.uncertain)[0]:
        log["cmp"].append(("prune", float(w1[e]), opt["edge_prune_threshold"]))
    pruned = drop.copy()
    nodes, w2, p2 = lm_pass(nodes, g, opt, pruned, ld, log)
    weight = np.where(pruned, w1, w2)
    return dict(nodes=nodes, weight=weight, pruned=pruned, passes=[p1, p2], n_pruned=int(drop.sum()), log=log)


def check_margins(res):
    """no decision of the run is a near-tie: every rho at least 1e-3 from 0, every comparison off its threshold by a factor >= 2"""
    for rho in res["log"]["rho"]:
        assert abs(rho) >= 1e-3, "rho = %g is within 1e-3 of 0" % rho
    for kind, lhs, rhs in res["log"]["cmp"]:
        assert lhs <= 0.5 * rhs or lhs >= 2.0 * rhs, "%s: %g against %g is within a factor 2" % (kind, lhs, rhs)


def information(rng, n_points=300, radius=30.0):
    """sum G^T G over random points within `radius`, G = [-[t]x | I] (iba_scan_information's form: [5, 5] is the count)"""
    t = rng.uniform(-1, 1, size=(n_points, 3))
    t = t / np.maximum(np.linalg.norm(t, axis=1, keepdims=True), 1e-9) * (radius * rng.uniform(0, 1, size=(n_points, 1)) ** (1 / 3))
    G = np.zeros((n_points, 3, 6))
    G[:, 0, 1], G[:, 0, 2], G[:, 1, 0], G[:, 1, 2], G[:, 2, 0], G[:, 2, 1] = t[:, 2], -t[:, 1], -t[:, 2], t[:, 0], t[:, 1], -t[:, 0]
    G[:, 0, 3] = G[:, 1, 4] = G[:, 2, 5] = 1.0
    I = np.einsum("nki,nkj->ij", G, G)
    return I


def make_graph(N, loops=0, false_loops=0, seed=0, rot_noise=1e-3, trans_noise=1e-2, false_offset=5.0, noise_free=False, min_gap=8):
    """A smooth random trajectory G_i, chain edges (i, i + 1) with X = G_(i+1)^-1 G_i times small noise, `loops` true and `false_loops` false
    (off by false_offset metres) uncertain edges between distant nodes; the initial nodes are the integrated noisy odometry."""
    rng = np.random.default_rng(seed)
    truth = np.zeros((N, 4, 4))
    truth[0] = np.eye(4)
    yaw = 0.0
    for i in range(1, N):
        yaw = 0.9 * yaw + rng.normal(0, 0.02)
        step = T_of(np.array([rng.normal(0, 0.003), rng.normal(0, 0.003), yaw, 1.0 + rng.normal(0, 0.05), rng.normal(0, 0.02), rng.normal(0, 0.01)]))[0]
        truth[i] = truth[i - 1] @ step

    def measure(s, t, offset=None):
        X = np.linalg.inv(truth[t]) @ truth[s]
        if not noise_free:
            X = X @ T_of(np.concatenate([rng.normal(0, rot_noise, 3), rng.normal(0, trans_noise, 3)]))[0]
        if offset is not None:
            X = X @ T_of(np.concatenate([np.zeros(3), offset]))[0]
        X[3] = [0, 0, 0, 1]
        return X

    src, tgt, X, info, unc = [], [], [], [], []
    for i in range(N - 1):
        src.append(i); tgt.append(i + 1); X.append(measure(i, i + 1)); info.append(information(rng)); unc.append(False)
    for k in range(loops + false_loops):
        while True:
            a, b = sorted(rng.integers(0, N, size=2).tolist())
            if b - a >= min(min_gap, max(N - 1, 1)) and (a, b) not in zip(src, tgt):
                break
        off = None
        if k >= loops:
            d = rng.normal(size=3)
            off = false_offset * d / np.linalg.norm(d)
        src.append(a); tgt.append(b); X.append(measure(a, b, off)); info.append(information(rng)); unc.append(True)
    nodes = np.zeros((N, 4, 4))
    nodes[0] = truth[0]
    for i in range(N - 1):
        nodes[i + 1] = nodes[i] @ np.linalg.inv(X[i])
        nodes[i + 1, 3] = [0, 0, 0, 1]
    return Graph(nodes, src, tgt, X, info, unc, truth=truth)


def align_at(nodes, ref, k=0):
    """every pose left-multiplied so that node k coincides with ref[k]"""
    C = ref[k] @ np.linalg.inv(nodes[k])
    return np.einsum("ij,njk->nik", C, nodes)


def case_graph(N, cross=(), missing_chain=(), seed=0, reverse=()):
    """A noisy graph on a smooth trajectory with the chain edges (i, i + 1) except those starting at `missing_chain`, then the cross edges
    (uncertain) as listed — (s, t) is kept in the order given, so t < s is an edge against the chain; chain edges at `reverse` are stored (i + 1, i)."""
    base = make_graph(N, seed=seed)
    rng = np.random.default_rng(1000 + seed)
    src, tgt, X, info, unc = [], [], [], [], []

    def add(s, t, u):
        M = np.linalg.inv(base.truth[t]) @ base.truth[s] @ T_of(np.concatenate([rng.normal(0, 2e-3, 3), rng.normal(0, 3e-2, 3)]))[0]
        M[3] = [0, 0, 0, 1]
        src.append(s); tgt.append(t); X.append(M); info.append(information(rng, 60)); unc.append(u)

    for i in range(N - 1):
        if i in missing_chain:
            continue
        add(*((i + 1, i) if i in reverse else (i, i + 1)), False)
    for s, t in cross:
        add(s, t, True)
    nodes = base.truth.copy()
    for i in range(N):
        nodes[i] = nodes[i] @ T_of(np.concatenate([rng.normal(0, 3e-3, 3), rng.normal(0, 5e-2, 3)]))[0]
        nodes[i, 3] = [0, 0, 0, 1]
    return Graph(nodes, src, tgt, X, info, unc, truth=base.truth)


# (name, N, cross edges, missing chain edges, segment, separator cap or None): the shapes of the solve and plan tests
SOLVE_CASES = [("n%d" % n, n, (), (), 4, None) for n in (1, 2, 3, 4, 5, 8, 9, 17)] + [
    ("cross_sep_sep", 17, ((4, 12),), (), 4, None),
    ("cross_same_run", 17, ((5, 7),), (), 4, None),
    ("cross_adjacent", 17, ((5, 6),), (), 4, None),
    ("cross_reversed", 17, ((14, 3),), (), 4, None),
    ("cross_shared_node", 17, ((2, 9), (9, 14)), (), 4, None),
    ("cross_ends", 17, ((0, 10), (6, 16)), (), 4, None),
    ("missing_chain", 17, (), (5,), 4, None),
    ("three_panels_ragged", 70, (), (), 4, None),        # 18 separators: 108 = 48 + 48 + 12
    ("k_doubles_once", 40, ((13, 30),), (), 4, 8),       # K = 4: 12 separators > 8; K = 8: 7
]

# (name, N, cross edges, segment, dict(K, separators, runs)): the shapes at which every loop of the solve iterates; their reference is sparse_solve.
#   rows_and_back_second_block: 2 and 7 cut the runs (1-3), (5-7) into lengths 1, 1, 2 beside (9-11) in forward block 0; 7 | 8 and 101 | 102 are
#   adjacent separators; (150, 21) is stored against the chain between runs of forward blocks 1 and 10. n = 474: 426 rows below the first
#   panel, a 14 x 14 grid of tiles with a ragged last one, all four waves of the separator solve, run and separator ids beyond 64.
#   at_the_cap / one_past_the_cap: the cap 1024 itself (no run at all, n = 6144 fills the separator solve's LDS) and the first doubling past it;
#   k_doubles_twice: 2050 -> 1025 -> 513 separators.
LARGE_SOLVE_CASES = [
    ("rows_and_back_second_block", 280, ((2, 7), (101, 102), (150, 21), (30, 200), (263, 58)), 4, dict(K=4, separators=79, runs=74)),
    ("at_the_cap", 1024, (), 1, dict(K=1, separators=1024, runs=0)),
    ("one_past_the_cap", 1025, (), 1, dict(K=2, separators=513, runs=512)),
    ("k_doubles_twice", 4100, (), 2, dict(K=8, separators=513, runs=513)),
]
_large_graphs = {}


def large_case_graph(name):
    """the graph of a LARGE_SOLVE_CASES entry, made once per process (the plan test and the device test share it; neither changes it)"""
    if name not in _large_graphs:
        _, N, cross, _, _ = next(c for c in LARGE_SOLVE_CASES if c[0] == name)
        _large_graphs[name] = case_graph(N, cross, seed=1)
    return _large_graphs[name]
