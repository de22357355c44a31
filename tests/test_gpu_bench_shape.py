"""The launch shapes bench.py times, against the oracle, inside the driver-run suite.

bench.py's headline evaluates 64 tight candidates on 200 keyframes x 10 k points x 2000 keypoints: 12 800 (candidate, keyframe) blocks, so the
shared-pair association runs as iba_assoc2_kernel<4, false, 256> (blocks of 256 threads from 1024 blocks up: csrc/iba_capi.hip, assoc2_threads),
the pair search as the one-wave iba_pairs_wave_kernel, the factor kernel on its plain (keyframe, candidate) grid. Here, on bench.py's own scene
(seed 0, built once for the module):
  * three batches bench.py times, each one fused evaluation on a fresh default handle: the headline (xs_all[0]: rng(0), 64 tight candidates, path 1),
    extras.wide_candidates (rng(7), 64 candidates uniform over the reference's search box: every candidate searches for itself, path 0) and two
    tight clusters of 32 tens of pixels apart (an optimiser's two polls: one pair list per group, path 2). Every counter of every candidate exact,
    f1 / f2 / C 1e-10, the normal-equation counts exact, and H, b, cost, chi^2 of EVERY candidate held to the long-double truth
    (tests/parity_gate.py) and within 2e-9 per entry of the double oracle. A candidate that misses either must pass the block-by-block explanation
    (tests/parity_explain.py) with flagged blocks, or come out of it clean (within 1e-10 of the double oracle), and only so many may: CAPS
    below, set from what an MI355X measured (MEASURED) plus a small margin.
    The worst device-vs-truth entry of H and of b over the batch stays within 2x its measured value;
  * the same bits on every path: the tight batch (path 1) and the clusters (path 2) against a handle where every candidate searches for itself
    (common_pairs = 0, anchored_lists = 0): partial blocks, cost tuples, H, b, cost, eval_cost — no tolerance at the timed shape;
  * 43 and 62 covisible keyframes per keyframe with the association FORCED to 256-thread blocks (IBA_ASSOC2_THREADS=256): the staging loop of the
    relative poses runs more than once per thread there (MANY);
  * three keyframes of 120 k points with 24 candidates: the dense-scan path of the pair search (blocks that test their boxes first, the 512-thread
    block kernel) under 256-thread association blocks."""
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import parity_explain  # noqa: E402
import parity_gate  # noqa: E402

pytestmark = pytest.mark.gpu
INT = ("valid_cnt_3d_2d", "cnt_3d_2d", "cnt_3d_3d", "valid_cnt_3d_3d", "valid_pl_3d_3d", "valid_pt_3d_3d", "frames_used", "n_corr")
NT = min(os.cpu_count() or 8, 16)   # oracle threads

# per batch, measured on an MI355X (two runs, the same figures): (candidates that needed the explanation, their flagged blocks, worst device-vs-truth
# entry of H, of b). tight: 26 of 64 explained, 2339 blocks, H 3.13e-8 (candidate 18), b 3.95e-6 (candidate 9: a cancelling entry; the double oracle
# is 5.6e-9 from the truth there). wide: 11, one of them clean (candidate 49), 206 blocks. clusters: 12, one of them clean (candidate 1), 687 blocks.
# The file took 212 s on 16 host cores.
MEASURED = {"tight": (26, 2339, 3.126e-8, 3.947e-6), "wide": (11, 206, 8.021e-8, 5.302e-8), "clusters": (12, 687, 1.573e-8, 1.719e-8)}
# (explained candidates, flagged blocks) allowed per batch: the measured counts + 3 candidates, + 10 % blocks
CAPS = {"tight": (29, 2580), "wide": (14, 230), "clusters": (15, 760)}


def _entries(g, o, rel):
    g, o = np.asarray(g, float).ravel(), np.asarray(o, float).ravel()
    big = np.max(np.abs(o))
    m = np.abs(o) > 1e-6 * big
    return float(np.max(np.abs(g - o)[m] / np.abs(o)[m])) <= rel and float(np.max(np.abs(g - o)[~m], initial=0.0)) <= rel * 1e-5 * big


def _cost_equal(a, b):
    for k in INT:
        assert getattr(a, k) == getattr(b, k), (k, getattr(a, k), getattr(b, k))
    assert abs(a.f1 - b.f1) <= 1e-10 * abs(b.f1) and abs(a.f2 - b.f2) <= 1e-10 * abs(b.f2)
    assert (np.isnan(a.C) and np.isnan(b.C)) or abs(a.C - b.C) <= 1e-10 * abs(b.C) + 1e-15


def _same_tuple(a, b):
    assert all(x == y or (x != x and y != y) for x, y in zip(a.as_dict().values(), b.as_dict().values())), (a.as_dict(), b.as_dict())


@pytest.fixture(scope="module")
def bench(pkg, synth, abi, ob):
    """bench.py's scene (seed 0), its three batches, the oracle, and the default handle's launch of each batch (evaluated once, on first use)"""
    prob, meta = synth.make_scene(n_frames=200, pts_per_frame=10000, n_keypoints=2000, seed=0)   # bench.py:184
    x_gt = meta["x_gt"]
    rng = np.random.default_rng(1)
    c2 = x_gt + np.array([0.02, -0.015, 0.01, 0.1, -0.08, 0.06, 0.2])                            # tens of pixels away (tests/test_gpu_common_pairs.py)
    batches = {"tight": synth.perturb(x_gt, np.random.default_rng(0), n=64),                      # bench.py:206, xs_all[0]
               "wide": x_gt[None, :] + np.random.default_rng(7).uniform(-1, 1, (64, 7)) * np.array([0.1, 0.1, 0.1, 0.3, 0.3, 0.3, 1.0]),   # bench.py:488
               "clusters": np.vstack([synth.perturb(x_gt, rng, n=32), synth.perturb(c2, rng, n=32)])}
    p = abi.reference_yaml_params()
    o = ob.Oracle(prob)
    handles, launches = [], {}

    def handle(**options):
        h = pkg.IbaHandle(prob, p, options=options or None)
        handles.append(h)
        return h

    def launch(name):
        """a fresh default handle's eval_full of one batch, and what the library reports about that launch"""
        if name not in launches:
            xs = batches[name]
            h = handle()
            cost, nrm = h.eval_full(xs)
            launches[name] = SimpleNamespace(h=h, xs=xs, cost=cost, nrm=nrm, partials=h.debug_last_partials(len(xs)), path=h.last_path,
                                             assoc2_threads=h.last_assoc2_threads, pairs_threads=h.last_pairs_threads, pair_lists=h.pair_lists,
                                             factor_ranges=h.debug_factor_ranges(len(xs)), cost_only=h.eval_cost(xs))
            print("\n%s: path %d, association blocks of %d threads, pair search %s, pair lists (overflowed, read, longest) %s"
                  % (name, h.last_path, launches[name].assoc2_threads, "one-wave (64)" if launches[name].pairs_threads == 64 else launches[name].pairs_threads,
                     launches[name].pair_lists), flush=True)
        return launches[name]

    yield SimpleNamespace(prob=prob, meta=meta, p=p, o=o, batches=batches, handle=handle, launch=launch)
    for h in handles:
        h.close()
    o.close()


def _against_the_oracle(bench, name):
    """every counter exact, f1 / f2 / C 1e-10, the normal equations of every candidate under the truth gate and 2e-9 of the double oracle — or
    explained, within CAPS; the eval_cost chain gives the same cost tuple"""
    r = bench.launch(name)
    xs, o, p = r.xs, bench.o, bench.p
    oc = o.eval_cost(p, xs, nthreads=NT)
    on = o.eval_normal(p, xs, nthreads=NT)
    tn = o.eval_normal_truth_batch(p, xs, nthreads=NT)
    explained, flagged, worst = [], [], {"H": (0.0, -1), "b": (0.0, -1)}
    for b in range(len(xs)):
        _cost_equal(r.cost[b], oc[b])
        assert r.nrm[b].counts() == on[b].counts() == tn[b].counts(), (name, b)
        ok, rep = parity_gate.check_normal_vs_truth(r.nrm[b], on[b], tn[b])
        for k in worst:
            if rep[k]["device"][0] > worst[k][0]:
                worst[k] = (rep[k]["device"][0], b)
        # device vs the double oracle: 2e-9 per entry (what a few ill-conditioned plane factors leave of two double evaluations: tests/parity_gate.py)
        near = (_entries(r.nrm[b].H_np(), on[b].H_np(), 2e-9) and _entries(r.nrm[b].b_np(), on[b].b_np(), 2e-9)
                and abs(r.nrm[b].cost - on[b].cost) <= 1e-9 * on[b].cost)
        if not (ok and near):
            # the device computes with ITS plane normals, which differ from the oracle's in the last bits, and an ill-conditioned block amplifies
            # that (a block with |r| = 2e4 px moves the cost itself by 2e-9 of the total): the block-by-block explanation must account for it.
            # "clean" instead: H and b within 1e-10 per entry of the double oracle, the strict gate of rounds 1-5 — a miss of the truth gate by the
            # gap of its bar max(1e-10, 1.5 x the oracle's error) where that error is itself near 1e-10; accepted for H and b only, and counted
            res = parity_explain.explain(r.h, o, p, xs[b], nthreads=NT)
            strict = res["status"] == "clean" and near and set(rep["failed"]) <= {"H", "b"}
            assert (res["status"] == "explained" and res["flagged"] > 0) or strict, (name, b, rep, near, res)
            explained.append(b)
            flagged.append(res["flagged"])
            print("%s: candidate %d explained (truth gate missed: %s, 2e-9 of the double oracle: %s): %d flagged block(s), device vs truth H %.2e "
                  "b %.2e, double oracle vs truth H %.2e b %.2e" % (name, b, rep["failed"] or "-", "kept" if near else "missed", res["flagged"],
                                                                     rep["H"]["device"][0], rep["b"]["device"][0], rep["H"]["oracle"][0], rep["b"]["oracle"][0]))
    print("%s: %d of %d candidates explained %s, %d flagged block(s) %s; worst device vs truth: H %.3e (candidate %d), b %.3e (candidate %d)"
          % (name, len(explained), len(xs), explained, sum(flagged), flagged, worst["H"][0], worst["H"][1], worst["b"][0], worst["b"][1]), flush=True)
    # the cost-only chain at the same launch shape: the same cost tuple
    for a, b in zip(r.cost_only, r.cost):
        for k in INT:
            assert getattr(a, k) == getattr(b, k)
        assert a.C == b.C and abs(a.f1 - b.f1) <= 1e-13 * b.f1
    parity_gate.explained_within(explained, flagged, *CAPS[name], what=name)
    wH, wb = MEASURED[name][2:]
    assert worst["H"][0] <= 2 * wH and worst["b"][0] <= 2 * wb, (name, worst, MEASURED[name])
    return r


def test_the_headline_launch_against_the_oracle(bench):
    r = bench.launch("tight")
    assert r.path == 1 and r.assoc2_threads == 256, (r.path, r.assoc2_threads)
    assert r.pairs_threads == 64   # the one-wave pair search bench.py times
    assert r.factor_ranges == 0    # (the default factor kernel: one wave per (keyframe, candidate))
    _against_the_oracle(bench, "tight")


def test_a_box_wide_batch_against_the_oracle(bench):
    """extras.wide_candidates: windows of tens of pixels, every candidate searches for itself (iba_assoc_kernel)"""
    assert bench.launch("wide").path == 0
    _against_the_oracle(bench, "wide")


def test_two_tight_clusters_against_the_oracle(bench):
    """two groups, one pair list each per keyframe: 2 x 200 lists read, none overflowed (a stale slot of an earlier batch would add lists: this
    handle has evaluated only this batch)"""
    r = bench.launch("clusters")
    assert r.path == 2, r.path
    assert r.pair_lists[:2] == (0, 400) and r.pair_lists[2] > 0, r.pair_lists
    _against_the_oracle(bench, "clusters")


def test_every_path_gives_the_same_bits(bench):
    """the direct guard of the association: the tight batch (path 1) and the two clusters (path 2) give the bits of a handle where every candidate
    searches for itself (path 0) — partial blocks, cost tuples, the normal equations, the cost-only chain"""
    h0 = bench.handle(common_pairs=0, anchored_lists=0)
    for name, want in (("tight", 1), ("clusters", 2)):
        r = bench.launch(name)
        assert r.path == want
        xs = r.xs
        c0, n0 = h0.eval_full(xs)
        p0 = h0.debug_last_partials(len(xs))
        assert h0.last_path == 0
        assert np.array_equal(p0, r.partials), (name, np.argwhere(p0 != r.partials)[:5])
        for a, b in zip(c0, r.cost):
            _same_tuple(a, b)
        for a, b in zip(n0, r.nrm):
            assert np.array_equal(a.H_np(), b.H_np()) and np.array_equal(a.b_np(), b.b_np()) and a.cost == b.cost and a.counts() == b.counts(), name
        a0 = h0.eval_cost(xs)
        assert h0.last_path == 0
        for a, b, c in zip(a0, r.cost_only, c0):
            _same_tuple(a, b)
            for k in INT:
                assert getattr(a, k) == getattr(c, k)
            assert a.C == c.C and abs(a.f1 - c.f1) <= 1e-13 * c.f1


@pytest.mark.parametrize("n_covis", [43, 62])
def test_many_covisible_keyframes_on_256_thread_association_blocks(pkg, synth, abi, ob, n_covis, monkeypatch):
    prob, meta = synth.make_scene(n_frames=n_covis + 4, pts_per_frame=2000, n_keypoints=600, seed=47, n_covis=n_covis, new_mappoints=100, scan_kp=140)
    p = abi.reference_yaml_params()
    monkeypatch.setenv("IBA_ASSOC2_THREADS", "256")
    h = pkg.IbaHandle(prob, p)
    monkeypatch.delenv("IBA_ASSOC2_THREADS")
    o = ob.Oracle(prob)
    xs = np.vstack([meta["x_gt"][None], synth.perturb(meta["x_gt"], np.random.default_rng(47), n=5)])
    cost, nrm = h.eval_full(xs)
    assert h.last_path == 1 and h.last_assoc2_threads == 256
    for a, b in zip(cost, o.eval_cost(p, xs, nthreads=8)):
        _cost_equal(a, b)
    assert cost[0].cnt_3d_2d > 4 * cost[0].n_corr   # matches in the slots beyond the 42nd
    for a, b in zip(nrm, o.eval_normal(p, xs, nthreads=8)):
        assert a.counts() == b.counts() and np.max(np.abs(a.H_np() - b.H_np())) <= 1e-8 * np.abs(b.H_np()).max()
    # the same candidates on the default handle (512-thread blocks at this size): the same bits
    h2 = pkg.IbaHandle(prob, p)
    c2, n2 = h2.eval_full(xs)
    assert h2.last_assoc2_threads == 512
    for a, b in zip(cost, c2):
        assert a.as_dict() == b.as_dict() or all(x == y or (x != x and y != y) for x, y in zip(a.as_dict().values(), b.as_dict().values()))
    for a, b in zip(nrm, n2):
        assert np.array_equal(a.H_np(), b.H_np()) and np.array_equal(a.b_np(), b.b_np())
    h.close(); h2.close()


def test_dense_scans_on_256_thread_association_blocks(pkg, synth, abi, ob, monkeypatch):
    prob, meta = synth.make_scene(n_frames=3, pts_per_frame=120000, n_keypoints=2000, seed=5)
    p = abi.reference_yaml_params()
    monkeypatch.setenv("IBA_ASSOC2_THREADS", "256")
    h = pkg.IbaHandle(prob, p)
    monkeypatch.delenv("IBA_ASSOC2_THREADS")
    o = ob.Oracle(prob)
    xs = synth.perturb(meta["x_gt"], np.random.default_rng(6), n=24)
    cost, nrm = h.eval_full(xs)
    assert h.last_path == 1 and h.last_assoc2_threads == 256 and h.last_pairs_threads == 0   # (dense scans: the 512-thread block kernel)
    for a, b in zip(cost, o.eval_cost(p, xs, nthreads=NT)):
        _cost_equal(a, b)
    for a, b in zip(nrm, o.eval_normal(p, xs, nthreads=NT)):
        assert a.counts() == b.counts() and np.max(np.abs(a.H_np() - b.H_np())) <= 1e-8 * np.abs(b.H_np()).max()
    h.close()
