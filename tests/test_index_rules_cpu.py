"""CPU tier of the device index build (iba_submap_handle): the numpy restatement of the build rules, LEVEL BY LEVEL as csrc/iba_index_kernels.hpp
states them (tests/index_ref.py: np.lexsort on (index, value with the zeros merged) per segment), against the tree the library's host build produces
(build_tree of csrc/iba_build.hpp through the host-only iba_debug_build_tree) — permutation, nodes and depth as raw bytes. The clouds are those of the
GPU tier (tests/test_gpu_submap_handle.py): every edge of tree_depth_for, Ppad and the 64-point chunk, a lattice full of ties, both signed zeros, and a
cloud at the depth cap. No GPU is touched."""
import numpy as np

import index_ref as X


def _same_tree(pkg, pts, what):
    host = pkg.debug_build_tree(pts)
    ref = X.build(pts)
    assert host["depth"] == ref["depth"] == X.depth_for(len(pts)), (what, host["depth"], ref["depth"])
    for key in ("perm", "node_dim", "node_split"):
        assert host[key].dtype == ref[key].dtype and host[key].shape == ref[key].shape, (what, key)
    bad = np.flatnonzero((host["node_dim"] != ref["node_dim"]) | (host["node_split"].view(np.uint32) != ref["node_split"].view(np.uint32)))
    assert len(bad) == 0, (what, "first differing node (heap index)", int(bad[0]), int(host["node_dim"][bad[0]]), float(host["node_split"][bad[0]]), int(ref["node_dim"][bad[0]]), float(ref["node_split"][bad[0]]))
    assert host["perm"].tobytes() == ref["perm"].tobytes(), (what, "first differing tree position", int(np.flatnonzero(host["perm"] != ref["perm"])[0]))
    return ref


def test_the_clouds_hit_every_edge(synth):
    cl = X.clouds(synth)
    sizes = {n: len(c) for n, c in cl.items()}
    print("index-figures", sizes)
    assert sizes["P=0"] == 0 and all(sizes["P=%d" % t] == t for t in X.P_EDGES)
    assert sizes["P%4"] % 4 != 0 and sizes["P%4"] > 1000
    assert sizes["deep"] > 49152 and X.depth_for(sizes["deep"]) == 11
    assert [X.depth_for(p) for p in (0, 1, 24, 25, 49, 50, 63, 64, 65)] == [0, 0, 0, 1, 1, 2, 2, 2, 2]
    z = cl["zeros"][:, 1].view(np.uint32)
    assert (z == 0x80000000).sum() > 50 and (z == 0).sum() > 50, ((z == 0x80000000).sum(), (z == 0).sum())   # -0.0f and +0.0f both occur after the narrowing
    lat = cl["lattice"]
    assert max(len(np.unique(lat[:, a])) for a in range(3)) < len(lat) // 4                                      # many equal coordinates: ties go to the index


def test_the_restatement_equals_the_host_build(pkg, synth):
    for name, pts in X.clouds(synth).items():
        ref = _same_tree(pkg, pts, name)
        if name == "zeros":       # the tie rule was really exercised: some node splits along y AT a zero, with zeros of both signs in its segment
            y_nodes = np.flatnonzero((ref["node_dim"] == 1) & (ref["node_split"] == 0))
            assert len(y_nodes) > 0


def test_ties_and_signed_zeros_alone(pkg):
    rng = np.random.default_rng(5)
    for P in (25, 49, 50, 97, 200, 1000):
        pts = rng.integers(-2, 3, (P, 3)).astype(np.float32)                   # five values per axis: almost every comparison is a tie
        pts[rng.random((P, 3)) < 0.3] *= np.float32(-1.0)                       # ... and the zeros carry both signs
        assert (pts.view(np.uint32) == 0x80000000).any() and (pts.view(np.uint32) == 0).any()
        _same_tree(pkg, pts, "ties P=%d" % P)
    one = np.zeros((300, 3), np.float32); one[::2] = -0.0                        # every extent is zero: dimension 0, the order is the index alone
    ref = _same_tree(pkg, one, "all zeros")
    assert (ref["node_dim"] == 0).all() and np.array_equal(ref["perm"], np.arange(300))


def test_ordered_key():
    v = np.array([-np.inf, -3.5, -1e-45, -0.0, 0.0, 1e-45, 2.0, np.inf], np.float32)
    k = X.ordered(v)
    assert k[3] == k[4] and (np.diff(k[[0, 1, 2, 3, 5, 6, 7]].astype(np.int64)) > 0).all()
