"""Pins the oracle's kd-tree/kNN restatement (oracle/oracle_kdtree.hpp) to the reference's vendored
nanoflann v1.5.0: (1) committed golden vectors generated from the reference's own headers
(tests/golden/make_golden.py), (2) seeded clouds against nanoflann's recorded outputs on them (tests/golden/knn_nanoflann_v150_live.npz)
and, when oracle/_ref is built, against that build live."""
import os

import numpy as np
import pytest

GOLD = os.path.join(os.path.dirname(__file__), "golden", "knn_nanoflann_v150.npz")
LIVE = os.path.join(os.path.dirname(__file__), "golden", "knn_nanoflann_v150_live.npz")
CASES = ["2d_leaf10", "3d_leaf30", "3d_leaf30_small", "2d_leaf10_dups"]


@pytest.mark.parametrize("name", CASES)
@pytest.mark.parametrize("k", [1, 30])
def test_oracle_knn_matches_nanoflann_golden(ob, name, k):
    z = np.load(GOLD)
    dim, leaf = (int(v) for v in z[f"{name}_meta"])
    idx, d2, cnt = ob.knn("oracle", dim, z[f"{name}_pts"], leaf, z[f"{name}_q"], k)
    # bit-exact: indices (including tie order: first visited wins, nanoflann.hpp:213), squared distances, counts
    assert np.array_equal(cnt, z[f"{name}_k{k}_cnt"])
    assert np.array_equal(idx, z[f"{name}_k{k}_idx"])
    assert np.array_equal(d2, z[f"{name}_k{k}_d2"])


def live_cases():
    """The seeded clouds of the live comparison: (key, dim, leaf, pts, queries, k). tests/golden/make_golden.py live records
    nanoflann's (idx, d2, cnt) for each of them, with a hash of the inputs."""
    rng = np.random.default_rng(1)
    for dim, leaf in ((2, 10), (3, 30), (3, 1)):
        for n in (1, 7, 31, 2500):
            pts = rng.normal(size=(n, dim)).astype(np.float32).astype(np.float64)
            if n > 100:
                pts[50:60] = pts[40:50]
            q = np.vstack([rng.normal(size=(64, dim)), pts[: min(n, 32)]])
            for k in (1, 30):
                yield "d%d_leaf%d_n%d_k%d" % (dim, leaf, n, k), dim, leaf, pts, q, k


def inputs_sha256(*arrays):
    import hashlib
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a, np.float64).tobytes())
    return np.frombuffer(h.digest(), np.uint8)


def test_oracle_knn_matches_live_reference_build(ob):
    z = np.load(LIVE)
    live = ob.ref_lib() is not None
    for key, dim, leaf, pts, q, k in live_cases():
        assert np.array_equal(inputs_sha256(pts, q), z[key + "_in_sha256"]), "inputs differ from the recorded ones: rerun tests/golden/make_golden.py live"
        a = ob.knn("oracle", dim, pts, leaf, q, k)
        assert all(np.array_equal(x, z[key + "_" + f]) for x, f in zip(a, ("idx", "d2", "cnt"))), key
        if live:
            b = ob.knn("ref", dim, pts, leaf, q, k)
            assert all(np.array_equal(x, y) for x, y in zip(a, b)), key


def test_knn_is_exact_vs_brute_force(ob):
    rng = np.random.default_rng(2)
    pts = (rng.normal(size=(3000, 3)) * [20, 8, 1.5]).astype(np.float32).astype(np.float64)
    q = rng.normal(size=(50, 3)) * [20, 8, 1.5]
    idx, d2, cnt = ob.knn("oracle", 3, pts, 30, q, 30)
    for i in range(len(q)):
        d = ((q[i] - pts) ** 2).sum(1)
        o = np.argsort(d, kind="stable")[:30]
        assert np.array_equal(np.sort(idx[i]), np.sort(o))
        assert np.allclose(d2[i], d[o], rtol=1e-14)


def test_knn_empty_and_tiny(ob):
    idx, d2, cnt = ob.knn("oracle", 3, np.zeros((0, 3)), 30, np.zeros((2, 3)), 5)
    assert np.all(cnt == 0)
    idx, d2, cnt = ob.knn("oracle", 2, np.array([[1.0, 2.0], [3.0, 4.0]]), 10, np.array([[0.0, 0.0]]), 5)
    assert cnt[0] == 2 and list(idx[0][:2]) == [0, 1] and d2[0][0] == 5.0


def test_oracle_knn_on_the_kitti_sized_fixture(ob, synth):
    """tests/golden/knn_nanoflann_v150_big.npz (round 5): nanoflann's kNN(30) / 1-NN INDICES on a 40 000-point scan that is regenerated from its
    seed (hash-checked). The restated tree must return the same indices; the GPU tier runs the device searches against the same file."""
    import hashlib
    z = np.load(os.path.join(os.path.dirname(__file__), "golden", "knn_nanoflann_v150_big.npz"))
    nf, ppf, nk, seed, nm, sk = (int(v) for v in z["scene"])
    prob, _ = synth.make_scene(n_frames=nf, pts_per_frame=ppf, n_keypoints=nk, seed=seed, new_mappoints=nm, scan_kp=sk)
    pts = prob.frame_points(0).astype(np.float32)
    assert np.array_equal(np.frombuffer(hashlib.sha256(pts.tobytes()).digest(), np.uint8), z["pts_sha256"])
    p64 = pts.astype(np.float64)
    idx, d2, cnt = ob.knn("oracle", 3, p64, 30, p64[z["self_sel"].astype(np.int64)], 30)
    assert np.all(cnt == 30) and np.array_equal(idx, z["self_k30_idx"].astype(np.uint32))
    i1, d1, _ = ob.knn("oracle", 3, p64, 30, z["q"], 1)
    assert np.array_equal(i1[:, 0], z["q_k1_idx"].astype(np.uint32))
