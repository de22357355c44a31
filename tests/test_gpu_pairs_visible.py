"""The visible-chunk list of the shared pair search (iba_vis_list_kernel: the chunks a camera near an anchor transform can see, built once
and walked by iba_pairs_wave_kernel instead of the whole (chunks, keyframes) grid) against the full grid (IBA_PAIRS_VISIBLE=0): the
partial blocks of eval_full_partial bit for bit and the per-keyframe pair lists as sorted sets, over the shapes and call sequences the
list has special cases for. The wave still tests its chunk with the call's own bound, so the list must never show in a result.
A rebuild is launched behind the search that found its batch outside the bound (that search runs the full grid) and waits for nothing:
the next search walks the list. IBA_PAIR_MEMO=0 keeps every call searching where a case needs two searches of one batch."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def _handle(pkg, prob, p, monkeypatch, env=None, mode=1, **opts):
    monkeypatch.setenv("IBA_DEBUG_ENV", "1")
    for k, v in (env or {}).items():
        monkeypatch.setenv(k, str(v))
    h = pkg.IbaHandle(prob, p, options=dict(common_pairs=mode, **opts))
    for k in (env or {}):
        monkeypatch.delenv(k)
    return h


def _partials(pkg, h, xs):
    """the 64-double partial blocks of iba_eval_full_partial, as bytes"""
    import torch
    ts = torch.cuda.Stream()
    with torch.cuda.stream(ts):
        d = torch.full((len(xs) * pkg.partial_stride(),), float("nan"), dtype=torch.float64, device="cuda:0")
        h.eval_full_partial(xs, d.data_ptr(), ts.cuda_stream)
        ts.synchronize()
        return d.cpu().numpy().tobytes()


def _lists(h, n_frames, slots=(-1,)):
    out = []
    for s in slots:
        for f in range(n_frames):
            lst = h.pair_list(f, s).astype(np.int64)
            out.append(np.sort(lst[:, 0] * (1 << 20) + lst[:, 1]).tobytes())
    return out


def _pair(pkg, prob, p, monkeypatch, env=None, **kw):
    """(default handle, the same with the full grid forced)"""
    return (_handle(pkg, prob, p, monkeypatch, env, **kw), _handle(pkg, prob, p, monkeypatch, dict(env or {}, IBA_PAIRS_VISIBLE=0), **kw))


def _same_call(pkg, prob, hv, h0, xs, slots=(-1,)):
    a, b = _partials(pkg, hv, xs), _partials(pkg, h0, xs)
    assert a == b
    assert hv.last_path == h0.last_path and hv.last_pairs_threads == h0.last_pairs_threads
    assert h0.pairs_visible[2] == 0 and h0.pairs_visible[1] == 0
    if hv.last_path > 0:
        assert _lists(hv, prob.n_frames, slots) == _lists(h0, prob.n_frames, slots)
    return a


def _edit_scan(abi, prob, frame, edit):
    """the problem with the scan of one keyframe replaced by edit(points (n, 3))"""
    a = dict(prob.arrays)
    off = a["pt_offset"].astype(np.int64)
    pts = a["pts_xyz"].reshape(-1, 3)
    new = np.ascontiguousarray(edit(pts[off[frame]:off[frame + 1]].copy()))
    a["pts_xyz"] = np.concatenate([pts[:off[frame]], new, pts[off[frame + 1]:]]).reshape(-1)
    off[frame + 1:] += len(new) - (off[frame + 1] - off[frame])
    a["pt_offset"] = off.astype(np.uint64)
    return abi.Problem(**a)


@pytest.fixture(scope="module")
def scene(synth):
    return synth.make_scene(n_frames=10, pts_per_frame=2001, n_keypoints=300, seed=5)   # (2001: not a multiple of 64)


NOMEMO = dict(IBA_PAIR_MEMO=0)


def test_tight_batches_and_groups(pkg, synth, abi, scene, monkeypatch):
    """1, 3 and 24 tight candidates and two clusters of 12 (groups, path 2): each twice on fresh handles — the first search launches the list,
    the second walks it; then all four in a row on default handles (pair-list reuse live: a covered batch runs no search at all)"""
    prob, meta = scene
    p = abi.reference_yaml_params()
    rng = np.random.default_rng(3)
    hn = _handle(pkg, prob, p, monkeypatch, mode=0)   # every candidate searches for itself
    tight = synth.perturb(meta["x_gt"], rng, n=24)
    c2 = meta["x_gt"] + np.array([0.02, -0.015, 0.01, 0.1, -0.08, 0.06, 0.2])
    two = np.vstack([synth.perturb(meta["x_gt"], rng, n=12), synth.perturb(c2, rng, n=12)])
    batches = ((tight[:1], 1), (tight[:3], 1), (tight, 1), (two, 2))
    for xs, path in batches:
        hv, h0 = _pair(pkg, prob, p, monkeypatch, NOMEMO)
        for call in range(3):
            a = _same_call(pkg, prob, hv, h0, xs, slots=(0, 1, 2, 3) if path == 2 else (-1,))
            assert hv.last_path == path
            items, rebuilds, used, full = hv.pairs_visible
            assert rebuilds == 1 and used == (0 if call == 0 else 1)
            assert call == 0 or prob.n_frames <= items <= full
        if len(xs) == 3:
            assert _partials(pkg, hn, xs) == a and hn.last_path == 0
        hv.close(); h0.close()
    hv, h0 = _pair(pkg, prob, p, monkeypatch)
    for xs, path in batches + batches:
        _same_call(pkg, prob, hv, h0, xs, slots=(0, 1, 2, 3) if path == 2 else (-1,))
    assert hv.pairs_visible[1] >= 1
    for h in (hv, h0, hn):
        h.close()


def test_keyframe_behind_the_camera_and_short_keyframes(pkg, synth, abi, scene, monkeypatch):
    """a keyframe with no visible chunk (its first chunk is listed all the same: it clears the next call's counters — the list is walked
    twice), a keyframe of fewer than 64 points, point counts that are no multiple of 64"""
    prob, meta = scene
    p = abi.reference_yaml_params()
    rng = np.random.default_rng(7)

    def behind(q):
        q[:, 0] = -np.abs(q[:, 0]) - 1.0   # the camera looks along the scanner's +x
        return q
    prob2 = _edit_scan(abi, _edit_scan(abi, prob, 4, behind), 7, lambda q: q[:40])
    hv, h0 = _pair(pkg, prob2, p, monkeypatch)
    for call, n in enumerate((48, 48, 48, 9)):   # (48: too many for the reusable pair lists, so every call searches, on the counters the one before cleared)
        xs = synth.perturb(meta["x_gt"], rng, n=n)
        _same_call(pkg, prob2, hv, h0, xs)
        assert hv.last_path == 1 and (n == 9 or hv.pairs_visible[2] == (0 if call == 0 else 1))
        assert hv.pair_list(4).shape[0] == 0
    assert hv.pairs_visible[1] == 1 and hv.pairs_chunks_passing(0) >= prob2.n_frames
    hv.close(); h0.close()


def test_drifting_batches_rebuild_the_list(pkg, synth, abi, scene, monkeypatch):
    """eight batches whose centre walks away from the list's anchor: outside the bound the full grid runs, then the list is rebuilt
    (not before a few searches have passed); every call equals the full-grid handle's and a fresh handle's"""
    prob, meta = scene
    p = abi.reference_yaml_params()
    rng = np.random.default_rng(11)
    hv, h0 = _pair(pkg, prob, p, monkeypatch)
    step = np.array([2e-3, -1.5e-3, 1e-3, 0.015, -0.01, 0.01, 0.002])   # (one step stays inside a list's bound, three do not)
    used = []
    for k in range(8):
        xs = synth.perturb(meta["x_gt"] + k * step, rng, n=8)
        a = _same_call(pkg, prob, hv, h0, xs)
        used.append(hv.pairs_visible[2])
        hf = _handle(pkg, prob, p, monkeypatch)
        assert _partials(pkg, hf, xs) == a
        hf.close()
    assert hv.pairs_visible[1] >= 2, "the sequence left the bound: the list must have been rebuilt"
    assert used[0] == 0 and used[1] == 1 and 0 in used[2:] and 1 in used[5:], used
    hv.close(); h0.close()


def test_wide_batch_nan_and_new_parameters(pkg, synth, abi, scene, monkeypatch):
    prob, meta = scene
    p = abi.reference_yaml_params()
    rng = np.random.default_rng(13)
    tight = synth.perturb(meta["x_gt"], rng, n=24)
    box = meta["x_gt"][None, :] + rng.uniform(-1, 1, (24, 7)) * np.array([0.1, 0.1, 0.1, 0.3, 0.3, 0.3, 1.0])
    bad = tight.copy(); bad[5, 2] = np.nan
    for mode in (1, 2):   # 1: the planner leaves a box-wide batch to the per-candidate kernels; 2: it shares one search, far beyond the list's caps
        hv, h0 = _pair(pkg, prob, p, monkeypatch, NOMEMO, mode=mode)
        for xs, path, used in ((tight, 1, 0), (tight, 1, 1), (box, 0 if mode == 1 else 1, 0), (bad, 0, 0), (tight, 1, 1)):
            _same_call(pkg, prob, hv, h0, xs)
            assert hv.last_path == path and hv.pairs_visible[2] == used, "a box-wide batch or a NaN must not walk the list"
        assert hv.pairs_visible[1] == 1
        hv.close(); h0.close()
    # a new max_pixel_dist between two calls: a new list
    hv, h0 = _pair(pkg, prob, p, monkeypatch, NOMEMO)
    _same_call(pkg, prob, hv, h0, tight)
    _same_call(pkg, prob, hv, h0, tight)
    assert hv.pairs_visible[1:3] == (1, 1)
    p2 = abi.reference_yaml_params(); p2.max_pixel_dist = p.max_pixel_dist * 1.5
    hv.set_params(p2); h0.set_params(p2)
    _same_call(pkg, prob, hv, h0, tight)
    assert hv.pairs_visible[1:3] == (2, 0)
    _same_call(pkg, prob, hv, h0, tight)
    assert hv.pairs_visible[1:3] == (2, 1)
    hv.close(); h0.close()


def test_other_forms_of_the_pair_search(pkg, synth, abi, scene, monkeypatch):
    """the wave kernel in blocks of 256 and 512 threads walks the list too, and so does the 512-thread block kernel (pairs_dense_min forced
    low): its items are blocks of eight consecutive chunks, so its lists are the full grid's"""
    prob, meta = scene
    p = abi.reference_yaml_params()
    rng = np.random.default_rng(17)
    xs = synth.perturb(meta["x_gt"], rng, n=48)   # (too many for the reusable pair lists: every call searches)
    for env, form in ((dict(IBA_PAIRS_WAVE=256), 256), (dict(IBA_PAIRS_WAVE=512), 512), (dict(IBA_PAIRS_DENSE_MIN=1000), 0)):
        hv, h0 = _pair(pkg, prob, p, monkeypatch, env)
        for call in range(3):
            _same_call(pkg, prob, hv, h0, xs)
            items, rebuilds, used, full = hv.pairs_visible
            assert hv.last_pairs_threads == form and rebuilds == 1 and used == (0 if call == 0 else 1)
            assert call == 0 or (prob.n_frames <= items <= full and (form == 0 or items < full))
        hv.close(); h0.close()
