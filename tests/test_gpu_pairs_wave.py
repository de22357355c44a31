"""The shared pair search in one-wave blocks (iba_pairs_wave_kernel: one wave per 64-position culling chunk, the batch bound over the
chunk's own box) against the 512-thread block kernel it replaced (iba_pairs_kernel, kept behind IBA_PAIRS_WAVE=0 for the A/B):
  * the list it leaves (iba_debug_pair_list) holds every (scan point, keypoint) pair that one candidate's exact f64 test accepts —
    recomputed here in numpy with the reference's projection (v uses fx, iba_global.cpp:72-73) and the gate max_pixel_dist — and no
    pair twice;
  * every result bit is the same whichever form built the lists, over the shapes the search has special cases for."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

FORMS = (0, 64, 256, 512)   # IBA_PAIRS_WAVE: 0 = the block kernel, else the wave kernel in blocks of that many threads


def _handle(pkg, prob, p, form, monkeypatch, mode=2, **opts):
    """mode 2: every batch shares its pair search (one group); 1: the planner's default (groups, fall-backs)"""
    monkeypatch.setenv("IBA_DEBUG_ENV", "1")
    monkeypatch.setenv("IBA_PAIRS_WAVE", str(form))
    h = pkg.IbaHandle(prob, p, options=dict(common_pairs=mode, **opts))
    monkeypatch.delenv("IBA_PAIRS_WAVE")
    return h


def _accepted_pairs(ob, prob, x, frame, gate):
    """(original point index, keypoint index) pairs with the point in the image of candidate x and d^2 <= gate^2"""
    a = prob.arrays
    p0, p1 = int(a["pt_offset"][frame]), int(a["pt_offset"][frame + 1])
    k0, k1 = int(a["kp_offset"][frame]), int(a["kp_offset"][frame + 1])
    fx, _fy, cx, cy, W, H = a["intrinsics"].reshape(-1, 6)[frame]
    R, t, _s = ob.sim3exp(x)
    pts = a["pts_xyz"].reshape(-1, 3)[p0:p1].astype(np.float64)
    q = pts @ R.T + t
    with np.errstate(divide="ignore", invalid="ignore"):
        u = (fx * q[:, 0] + cx * q[:, 2]) / q[:, 2]
        v = (fx * q[:, 1] + cy * q[:, 2]) / q[:, 2]
    vis = np.flatnonzero((q[:, 2] > 0) & (u >= 0) & (u < W) & (v >= 0) & (v < H))
    kp = a["kp_uv"].reshape(-1, 2)[k0:k1].astype(np.float64)
    out = []
    for s in range(0, vis.size, 4096):
        i = vis[s:s + 4096]
        d2 = (kp[None, :, 0] - u[i, None]) ** 2 + (kp[None, :, 1] - v[i, None]) ** 2
        pi, ki = np.nonzero(d2 <= gate * gate)
        out.append(np.stack([i[pi], ki], 1))
    return np.concatenate(out).astype(np.int64) if out else np.zeros((0, 2), np.int64)


def _check_lists(ob, prob, h, xs, frames, gate):
    ov, _, _ = h.pair_lists
    assert ov == 0, "a list overflowed: the superset check needs whole lists"
    for f in frames:
        lst = h.pair_list(f).astype(np.int64)
        keys = lst[:, 0] * (1 << 20) + lst[:, 1]
        assert np.unique(keys).size == keys.size, ("duplicate pairs", f)
        have = set(keys.tolist())
        for x in xs:
            acc = _accepted_pairs(ob, prob, x, f, gate)
            miss = [tuple(r) for r in acc if int(r[0]) * (1 << 20) + int(r[1]) not in have]
            assert not miss, ("pairs the exact test accepts are missing from the list", f, miss[:5])
    return h.mean_pairs


@pytest.mark.parametrize("form", (64, 0))
def test_the_list_holds_every_accepted_pair_once(pkg, synth, abi, ob, scene_small, form, monkeypatch):
    p = abi.reference_yaml_params()
    rng = np.random.default_rng(31)
    scenes = [scene_small, synth.make_scene(n_frames=10, pts_per_frame=10000, n_keypoints=2000, seed=0)]   # (the second: the bench's keyframe shape)
    for prob, meta in scenes:
        h = _handle(pkg, prob, p, form, monkeypatch)
        xs = synth.perturb(meta["x_gt"], rng, n=64)
        h.eval_cost(xs)
        assert h.last_path == 1 and h.last_pairs_threads == form
        frames = range(0, prob.n_frames, 3)
        assert _check_lists(ob, prob, h, xs[::16], frames, p.max_pixel_dist) > 0
        # a wider batch: windows of several pixels and hard points
        xw = synth.perturb(meta["x_gt"], rng, rot=1e-3, trans=1e-2, scale_rel=2e-3, n=12)
        h.eval_cost(xw)
        _check_lists(ob, prob, h, xw[::4], frames, p.max_pixel_dist)
        h.close()


def _results(h, xs):
    c, n = h.eval_full(xs)
    parts = h.debug_last_partials(min(len(xs), 64))
    return [repr(a.as_dict()) for a in c], [(a.H_np(), a.b_np(), a.cost, a.counts()) for a in n], parts, h.last_path   # (repr: NaN == NaN)


def _same(r0, r1):
    assert r0[3] == r1[3]
    assert r0[0] == r1[0]
    assert r0[2].tobytes() == r1[2].tobytes()
    for a, b in zip(r0[1], r1[1]):
        assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes() and repr(a[2]) == repr(b[2]) and a[3] == b[3]


def _ab(pkg, prob, p, monkeypatch, batches, mode=2, **opts):
    hs = [_handle(pkg, prob, p, form, monkeypatch, mode, **opts) for form in FORMS]
    paths = []
    for xs in batches:
        rs = [_results(h, xs) for h in hs]
        for h, form in zip(hs, FORMS):
            assert h.last_path == 0 or h.last_pairs_threads == form
        for r in rs[1:]:
            _same(rs[0], r)
        paths.append(rs[0][3])
    for h in hs:
        h.close()
    return paths


def test_forms_give_the_same_bits(pkg, synth, abi, scene_small, monkeypatch):
    """a lone candidate (entrywise bound only), a tight batch, two groups (path 2), a reused inflated list, a small list capacity
    (overflow -> exact rescan)"""
    prob, meta = scene_small
    p = abi.reference_yaml_params()
    rng = np.random.default_rng(41)
    c1 = meta["x_gt"]
    c2 = c1 + np.array([0.02, -0.015, 0.01, 0.1, -0.08, 0.06, 0.2])
    tight = synth.perturb(c1, rng, n=64)
    two = np.vstack([synth.perturb(c1, rng, n=20), synth.perturb(c2, rng, n=21)])
    near = synth.perturb(c1, rng, rot=1e-4, trans=1e-3, scale_rel=3e-4, n=8)   # inside the first batch's inflated bound: reused lists
    paths = _ab(pkg, prob, p, monkeypatch, [tight[:1], tight, two, near, near[:3]], mode=1)
    assert paths[0] == 1 and paths[1] == 1 and paths[2] == 2
    _ab(pkg, prob, p, monkeypatch, [tight[:16]], pair_list_capacity=64)


def test_forms_give_the_same_bits_on_odd_shapes(pkg, synth, abi, monkeypatch):
    """scan sizes that are not a multiple of 64 (and one below 64) and a keyframe count that is not a multiple of 8"""
    p = abi.reference_yaml_params()
    rng = np.random.default_rng(43)
    for nf, npts in ((11, 3001), (5, 1000)):
        prob, meta = synth.make_scene(n_frames=nf, pts_per_frame=npts, seed=7)
        _ab(pkg, prob, p, monkeypatch, [synth.perturb(meta["x_gt"], rng, n=24)])
    prob, meta = synth.make_scene(n_frames=9, pts_per_frame=48, n_keypoints=40, seed=9)   # P < 64
    _ab(pkg, prob, p, monkeypatch, [synth.perturb(meta["x_gt"], rng, n=8)])


def test_forms_give_the_same_bits_on_dense_scans(pkg, synth, abi, monkeypatch):
    """keyframes of 120 k points (the reference's scan size): the dense order, box test before any point load"""
    p = abi.reference_yaml_params()
    prob, meta = synth.make_scene(n_frames=3, pts_per_frame=120000, seed=0)
    rng = np.random.default_rng(47)
    _ab(pkg, prob, p, monkeypatch, [synth.perturb(meta["x_gt"], rng, n=16)])
