"""CPU tier of the voxel down-sampling / merged sub-map clouds (iba_submap_build, include/iba_mi355x.h): symbols, the struct layout and the ABI
version through the ctypes mirror, the entry points on NULL arguments (answered without a device), and the numpy restatement
tests/submap_ref.py against known answers and against a differently written dict-of-lists implementation."""
import ctypes as C
import re

import numpy as np

import submap_ref as V

NAMES = ("iba_submap_build", "iba_submap_num", "iba_submap_n_voxels", "iba_submap_n_dropped", "iba_submap_xyz", "iba_submap_counts", "iba_submap_free")
I4 = np.eye(4)


# ---- 1. the boundary: these fail before the feature exists ----
def test_submap_symbols_are_declared_and_exported_and_the_abi_is_still_4(pkg, abi):
    pkg.build_extension()
    lib = pkg.load_library()
    hdr = open(pkg.HEADER_PATH).read()
    declared = set(re.findall(r"\b(iba_[a-z_0-9]+)\s*\(", hdr))
    for n in NAMES:
        assert n in declared, n
        assert getattr(lib, n) is not None, n
    assert int(re.search(r"#define IBA_ABI_VERSION (\d+)", hdr).group(1)) == pkg.ABI_VERSION == lib.iba_abi_version() == 4
    assert "typedef struct iba_submap_desc" in hdr and "typedef struct iba_submap_clouds iba_submap_clouds;" in hdr
    # the sentence that named these two as the caller's work is gone
    assert "voxel down-sampling and merged sub-map targets stay the caller's" not in hdr


def test_submap_desc_layout_matches_the_header(abi):
    D = abi.IbaSubmapDesc
    assert C.sizeof(D) == 40          # 2 x i32, 3 pointers, f64
    assert (D.struct_size.offset, D.n_members.offset, D.frames.offset, D.poses12.offset, D.out12.offset, D.voxel.offset) == (0, 4, 8, 16, 24, 32)
    assert abi.SUBMAP_MAX_BATCH == 4096 and abi.SUBMAP_MAX_AXIS_VOXELS == 131072


def test_null_handle_and_null_results_are_refused_without_a_device(pkg, abi):
    lib = pkg.load_library()
    lib.iba_submap_build.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.POINTER(C.c_void_p)]
    lib.iba_submap_num.argtypes = [C.c_void_p]; lib.iba_submap_num.restype = C.c_int32
    for f, rt in ((lib.iba_submap_n_voxels, C.c_int64), (lib.iba_submap_n_dropped, C.c_int64), (lib.iba_submap_xyz, C.c_void_p), (lib.iba_submap_counts, C.c_void_p)):
        f.argtypes = [C.c_void_p, C.c_int32]; f.restype = rt
    lib.iba_submap_free.argtypes = [C.c_void_p]; lib.iba_submap_free.restype = None
    d = (abi.IbaSubmapDesc * 1)()
    fr = np.zeros(1, np.int32); ps = np.eye(3, 4).ravel().copy()
    d[0].struct_size = C.sizeof(abi.IbaSubmapDesc); d[0].n_members = 1; d[0].frames = fr.ctypes.data; d[0].poses12 = ps.ctypes.data; d[0].voxel = 0.4
    res = C.c_void_p(None)
    assert lib.iba_submap_build(None, d, 1, C.byref(res)) == 1 and not res.value
    assert lib.iba_submap_build(None, None, 1, C.byref(res)) == 1
    assert lib.iba_submap_build(None, d, 1, None) == 1
    assert lib.iba_submap_num(None) == 0
    assert lib.iba_submap_n_voxels(None, 0) == -1 and lib.iba_submap_n_dropped(None, 0) == -1
    assert lib.iba_submap_xyz(None, 0) is None and lib.iba_submap_counts(None, 0) is None
    lib.iba_submap_free(None)


# ---- 2. the restatement against known answers ----
def _f32(a):
    return np.asarray(a, np.float32).reshape(-1, 3)


def test_lattice_points_have_the_known_voxel_means():
    # two points in every cell of a 3 x 2 x 2 lattice of unit voxels: (c + 0.25, c + 0.5) per axis, all exactly representable
    cells = [(i, j, k) for i in range(3) for j in range(2) for k in range(2)]
    pts = []
    for c in cells:
        pts += [np.array(c) + 0.25, np.array(c) + 0.5]
    pts = _f32(pts)
    r = V.build([(pts, I4)], 1.0)
    # minb = 0.25 - 0.5 = -0.25: index = floor(p + 0.25) = floor(c + 0.5) or floor(c + 0.75) = the cell
    assert np.array_equal(r["minb"], [-0.25] * 3)
    assert np.array_equal(r["idx"], np.array(cells)) and np.array_equal(r["count"], np.full(12, 2)) and r["n_dropped"] == 0
    assert np.array_equal(r["xyz"], np.array(cells) + 0.375)
    assert r["xyz"].dtype == np.float64 and r["count"].dtype == np.int32


def test_a_point_exactly_on_a_voxel_face_lands_in_the_upper_voxel():
    # min = 0 -> minb = -0.25 with voxel 0.5; p = 0.25 gives (0.25 + 0.25) / 0.5 = 1 exactly: voxel 1, not 0
    pts = _f32([[0, 0, 0], [0.25, 0, 0], [0.2499999, 0, 0], [0.75, 0, 0]])
    r = V.build([(pts, I4)], 0.5)
    d = (pts[:, 0].astype(np.float64) + 0.25) / 0.5
    assert d[1] == 1.0 and d[3] == 2.0 and d[2] < 1.0
    assert np.array_equal(r["idx"][:, 0], [0, 1, 2]) and np.array_equal(r["count"], [2, 1, 1])
    assert r["xyz"][1, 0] == 0.25 and r["xyz"][2, 0] == 0.75


def test_single_point_all_in_one_voxel_and_duplicates():
    one = V.build([(_f32([[1.5, -2.25, 3.0]]), I4)], 0.4)
    assert np.array_equal(one["xyz"], [[1.5, -2.25, 3.0]]) and np.array_equal(one["count"], [1]) and np.array_equal(one["idx"], [[0, 0, 0]])
    rng = np.random.default_rng(0)
    p = _f32(rng.uniform(0, 0.4, (100, 3)))
    allin = V.build([(p, I4)], 1.0)
    assert len(allin["xyz"]) == 1 and allin["count"][0] == 100
    acc = np.zeros(3)
    for row in p.astype(np.float64):
        acc = acc + row
    assert np.array_equal(allin["xyz"][0], acc / 100.0)              # the sequential sum, bit for bit
    dup = V.build([(_f32([[1, 2, 3]] * 7 + [[5, 5, 5]] * 3), I4)], 0.5)
    assert np.array_equal(dup["count"], [7, 3]) and np.array_equal(dup["xyz"], [[1, 2, 3], [5, 5, 5]])


def test_non_finite_points_are_dropped_and_counted():
    p = _f32([[0, 0, 0], [np.nan, 1, 1], [1, 1, 1], [1, np.inf, 1], [1, 1, -np.inf], [1.1, 1.1, 1.1]])
    r = V.build([(p, I4)], 0.5)
    assert r["n_dropped"] == 3 and r["count"].sum() == 3 and np.all(np.isfinite(r["xyz"]))
    # finite before, not finite after: the transform overflows
    big = _f32([[3e38, 0, 0], [1, 1, 1]])
    T = I4.copy(); T[0, 0] = 1e300
    r = V.build([(big, T)], 0.5)
    assert r["n_dropped"] == 1 and np.array_equal(r["count"], [1])
    # nothing kept: zero voxels, no error
    r = V.build([(_f32([[np.nan, 0, 0]]), I4), (np.zeros((0, 3), np.float32), I4)], 0.5)
    assert r["n_dropped"] == 1 and len(r["xyz"]) == 0 and len(r["count"]) == 0


def test_two_members_with_different_poses_fill_the_same_voxels():
    a = _f32([[0, 0, 0], [1, 0, 0], [0, 1, 0]])
    Tb = I4.copy(); Tb[:3, 3] = [10, 20, 30]
    b = _f32(a.astype(np.float64) - [10, 20, 30] + 0.125)            # lands 0.125 beside a's points under Tb
    r = V.build([(a, I4), (b, Tb)], 0.5)
    assert np.array_equal(r["count"], [2, 2, 2])
    assert np.array_equal(r["xyz"], np.array([[0, 0, 0], [0, 1, 0], [1, 0, 0]]) + 0.0625)
    # the order of the members is the order of the sum: swapping them may change low bits, never the set
    r2 = V.build([(b, Tb), (a, I4)], 0.5)
    assert np.array_equal(r2["count"], r["count"]) and np.array_equal(r2["idx"], r["idx"])
    # an output transform moves the averaged points by the expression of rule 1
    To = V.inverse34(Tb)
    assert np.array_equal(V.build([(a, I4), (b, Tb)], 0.5, To)["xyz"], V.apply(To, r["xyz"]))


def test_a_permutation_changes_low_bits_of_a_mean_but_never_the_voxel_set_or_the_counts():
    rng = np.random.default_rng(1)
    p = _f32(rng.normal(0, 0.5, (20000, 3)))          # dense: hundreds of points in the central voxels
    # (under the identity pose the sums of float32 values are exact in f64 and no order shows; a rotation gives q a full mantissa)
    c, s = np.cos(0.3), np.sin(0.3)
    T = np.array([[c, -s, 0, 0.1], [s, c, 0, -0.2], [0, 0, 1, 0.3]])
    r = V.build([(p, T)], 0.4)
    rp = V.build([(p[rng.permutation(len(p))], T)], 0.4)
    assert np.array_equal(r["idx"], rp["idx"]) and np.array_equal(r["count"], rp["count"])
    assert not np.array_equal(r["xyz"], rp["xyz"])
    assert np.max(np.abs(r["xyz"] - rp["xyz"])) <= 1e-13


def test_identity_pose_without_output_transform_is_load_pcd():
    rng = np.random.default_rng(2)
    p = _f32(rng.uniform(-20, 20, (5000, 3)))
    a, b = V.load_pcd(p, 0.4), V.build([(p, np.eye(3, 4))], 0.4, None)
    assert a["xyz"].tobytes() == b["xyz"].tobytes() and np.array_equal(a["count"], b["count"])
    assert a["count"].sum() == 5000 and len(a["xyz"]) < 5000
    # every averaged point lies inside its voxel (to rounding)
    lo = a["minb"] + a["idx"] * 0.4
    assert np.all(a["xyz"] >= lo - 1e-12) and np.all(a["xyz"] <= lo + 0.4 + 1e-12)


# ---- 3. the restatement against a dict-of-lists implementation written differently ----
def _brute(members, voxel, out=None):
    pts, dropped = [], 0
    for p, T in members:
        T = np.asarray(T, np.float64).reshape(-1, 4)
        for x, y, z in np.asarray(p, np.float32).reshape(-1, 3).astype(np.float64):
            with np.errstate(invalid="ignore", over="ignore"):
                q = [np.float64(((T[r][0] * x + T[r][1] * y) + T[r][2] * z) + T[r][3]) for r in range(3)]
            if all(np.isfinite(v) for v in (x, y, z)) and all(np.isfinite(v) for v in q):
                pts.append(q)
            else:
                dropped += 1
    if not pts:
        return [], [], dropped
    minb = [min(q[a] for q in pts) - 0.5 * voxel for a in range(3)]
    cells = {}
    for q in pts:
        cells.setdefault(tuple(int(np.floor((q[a] - minb[a]) / voxel)) for a in range(3)), []).append(q)
    xyz, cnt = [], []
    for key in sorted(cells):
        s = [np.float64(0.0)] * 3
        for q in cells[key]:
            s = [s[a] + q[a] for a in range(3)]
        m = [s[a] / float(len(cells[key])) for a in range(3)]
        if out is not None:
            O = np.asarray(out, np.float64).reshape(-1, 4)
            m = [((O[r][0] * m[0] + O[r][1] * m[1]) + O[r][2] * m[2]) + O[r][3] for r in range(3)]
        xyz.append(m); cnt.append(len(cells[key]))
    return xyz, cnt, dropped


def test_restatement_equals_the_dict_of_lists_brute_force_on_random_clouds():
    rng = np.random.default_rng(3)
    for trial in range(6):
        members = []
        for m in range(int(rng.integers(1, 4))):
            p = _f32(rng.normal(0, 2.0 + trial, (int(rng.integers(0, 1500)), 3)))
            if len(p) > 10 and trial % 2:
                p[rng.integers(0, len(p), 3)] = np.nan
            w = rng.normal(0, 0.3, 3); th = np.linalg.norm(w); k = w / th
            K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
            T = np.eye(4); T[:3, :3] = np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * K @ K; T[:3, 3] = rng.normal(0, 1, 3)
            members.append((p, T))
        voxel = float(rng.choice([0.1, 0.4, 2.0]))
        out = None if trial % 3 == 0 else V.inverse34(members[0][1])
        r = V.build(members, voxel, out)
        xyz, cnt, dropped = _brute(members, voxel, out)
        assert r["n_dropped"] == dropped and np.array_equal(r["count"], np.asarray(cnt, np.int32))
        assert r["xyz"].tobytes() == np.asarray(xyz, np.float64).reshape(-1, 3).tobytes()
