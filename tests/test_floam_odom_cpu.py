"""CPU tier of the lattice voxel filter and the local map's host-side rules: tests/floam_odom_ref.py (the restatement the GPU tier compares the device
with) against answers worked out by hand."""
import numpy as np

import floam_odom_ref as O
import submap_ref as V

I4 = np.eye(4)


def _f32(rows):
    return np.asarray(rows, np.float32).reshape(-1, 3)


def test_cells_are_anchored_at_the_origin_and_floor_towards_minus_infinity():
    # -0.1 / 0.4 = -0.25: cell -1, not 0 (a truncation would say 0)
    assert O.cells([[-0.1, 0.1, -0.4]], 0.4).tolist() == [[-1, 0, -1]]
    # exact multiples of the leaf sit in the cell they open; 0.5 is exact in binary, so the quotients are exact integers
    q = np.array([[-1.0, -0.5, 0.0], [0.5, 1.0, 1.5], [-0.0, 0.0, 0.25], [-0.25, 0.75, -0.75]])
    assert O.cells(q, 0.5).tolist() == [[-2, -1, 0], [1, 2, 3], [0, 0, 0], [-1, 1, -2]]
    # +0 and -0 share cell 0 and the largest double below 0 does not
    below = np.nextafter(0.0, -1.0)
    assert O.cells([[0.0, -0.0, below]], 0.4).tolist() == [[0, 0, -1]]
    # the lattice does not move with the cloud: the same point has the same cell whatever else is in the cloud (Open3D's grid does move)
    a = O.lattice([(_f32([[0.3, 0.3, 0.3]]), I4)], 0.4)
    b = O.lattice([(_f32([[0.3, 0.3, 0.3], [-7.7, 2.1, 0.0]]), I4)], 0.4)
    assert a["idx"].tolist() == [[0, 0, 0]] and [0, 0, 0] in b["idx"].tolist()
    assert V.indices(_f32([[0.3, 0.3, 0.3], [-7.7, 2.1, 0.0]]).astype(np.float64), 0.4)[0][0].tolist() != V.indices(_f32([[0.3, 0.3, 0.3]]).astype(np.float64), 0.4)[0][0].tolist()


def test_crop_keeps_both_faces():
    lo, hi = np.array([-1.0, -2.0, -3.0]), np.array([1.0, 2.0, 3.0])
    on = np.array([[-1.0, 0, 0], [1.0, 0, 0], [0, -2.0, 0], [0, 2.0, 0], [0, 0, -3.0], [0, 0, 3.0], [1.0, 2.0, 3.0], [-1.0, -2.0, -3.0]])
    assert O.inside(on, lo, hi).all()
    off = on.copy()
    for r in range(6):
        a = r // 2
        off[r, a] = np.nextafter(on[r, a], np.inf if on[r, a] > 0 else -np.inf)
    off[6, 1] = np.nextafter(2.0, np.inf); off[7, 2] = np.nextafter(-3.0, -np.inf)
    assert not O.inside(off, lo, hi).any()
    r = O.lattice([(_f32(on), I4), (_f32([[1.5, 0, 0], [np.nan, 0, 0], [0, 0, -3.5]]), I4)], 0.5, crop=(lo, hi))
    assert (r["n_cropped"], r["n_dropped"], int(r["count"].sum())) == (2, 1, 8)
    gone = O.lattice([(_f32(on), I4)], 0.5, crop=(np.full(3, 10.0), np.full(3, 11.0)))
    assert len(gone["xyz"]) == 0 and gone["n_cropped"] == 8 and gone["n_dropped"] == 0


def test_centroid_order_members_and_output_transform():
    a = _f32([[0.1, 0.1, 0.1], [0.3, 0.1, 0.1], [-0.1, 0.1, 0.1]])
    b = _f32([[0.2, 0.2, 0.2]])
    T = I4.copy(); T[:3, 3] = [0.0, 0.0, 0.125]
    r = O.lattice([(a, I4), (b, T)], 0.4)
    assert r["idx"].tolist() == [[-1, 0, 0], [0, 0, 0]] and r["count"].tolist() == [1, 3]
    qa, qb = a.astype(np.float64), b.astype(np.float64)
    want = ((qa[0] + qa[1]) + (qb[0] + [0.0, 0.0, 0.125])) / 3.0           # old members first, then the new one, one add at a time
    assert r["xyz"][1].tobytes() == want.tobytes()
    out = I4.copy(); out[:3, 3] = [1.0, 2.0, 3.0]
    moved = O.lattice([(a, I4), (b, T)], 0.4, out=out)
    assert moved["xyz"].tobytes() == V.apply(out, r["xyz"]).tobytes() and moved["idx"].tolist() == r["idx"].tolist()


def _rigid(deg_z, t):
    c, s = np.cos(np.radians(deg_z)), np.sin(np.radians(deg_z))
    T = np.eye(4); T[:3, :3] = [[c, -s, 0], [s, c, 0], [0, 0, 1]]; T[:3, 3] = t
    return T


def test_prediction_on_two_known_poses():
    # pure translations: the step 0 -> 1 is repeated
    A = _rigid(0, [1.0, 0.0, 0.0]); B = _rigid(0, [1.5, 0.25, 0.0])
    assert np.array_equal(O.predict(A, B), _rigid(0, [2.0, 0.5, 0.0]))
    # a turn of 90 degrees about z per step with a step of 1 m along the body's x: the third pose of the square
    A = _rigid(0, [0, 0, 0]); B = _rigid(90, [1.0, 0, 0])
    P = O.predict(A, B)
    assert np.allclose(P, _rigid(180, [1.0, 1.0, 0]), atol=1e-15)
    # T[-1] := T0 makes the first prediction the pose itself
    assert np.allclose(O.predict(B, B), B, atol=1e-15)
    assert np.allclose(O.rigid_inverse(B) @ B, np.eye(4), atol=1e-15)


def test_pass_schedule():
    assert O.pass_schedule(13) == [0, 11, 10, 9, 8, 7, 6, 5, 4, 3, 2, 2, 2]
    assert O.pass_schedule(1) == [0] and O.pass_schedule(3, init_passes=0) == [0, 2, 2]


def test_map_update_keeps_the_lattice_and_crops_around_the_pose():
    rng = np.random.default_rng(4)
    old_e = rng.uniform(-3, 3, (400, 3)).astype(np.float32); old_s = rng.uniform(-3, 3, (900, 3)).astype(np.float32)
    src_e = rng.uniform(-1, 1, (60, 3)).astype(np.float32); src_s = rng.uniform(-1, 1, (200, 3)).astype(np.float32)
    T = _rigid(10, [1.0, 0.5, 0.0])
    me, ms, e, s = O.update_map(old_e, old_s, src_e, src_s, T, 0.4, 2.0)
    assert me.dtype == np.float32 and len(me) == len(e["xyz"]) and e["n_cropped"] > 0 and s["n_cropped"] > 0
    lo, hi = O.crop_box(T, 2.0)
    assert np.array_equal(lo, [-1.0, -1.5, -2.0]) and np.array_equal(hi, [3.0, 2.5, 2.0])
    assert np.all(np.diff(e["idx"][:, 0]) >= 0)                         # cells ascending (ix, iy, iz): the map stays in lattice order
    # filtering the filtered map again with nothing new moves no cell: a centroid lies in its own cell (up to the float32 narrowing at a face)
    again = O.lattice([(me, I4)], 0.4)
    assert len(again["xyz"]) <= len(me) and len(again["xyz"]) >= len(me) - 2
    de, ds = O.downsample(src_e, src_s, 0.4)
    assert len(de) == len(O.lattice([(src_e, I4)], 0.4)["xyz"]) and len(ds) == len(O.lattice([(src_s, I4)], 0.8)["xyz"])
    ie, _ = O.init_map(src_e, src_s, T)
    assert ie.tobytes() == V.apply(T, src_e.astype(np.float64)).astype(np.float32).tobytes()


def test_the_reference_chain_follows_the_track():
    """the track the GPU tier runs, through the restatements alone: the final position error is at most a tenth of the track's length, and it is
    the figure the GPU tier's whole-track gate is built on (O.E_REF)"""
    cfg = O.TRACK
    scans = O.track_scans()
    steps = O.track(scans, I4, O.track_extract_options(), None, cfg["map_resolution"], cfg["crop_half"], cfg["init_passes"])
    length = cfg["step"] * (cfg["n_scans"] - 1)
    e_ref = O.track_error(steps[-1]["T"], cfg["n_scans"] - 1)
    print("floam-odom-figures e_ref", e_ref, "track length", length, "per step", [round(O.track_error(s["T"], k), 4) for k, s in enumerate(steps)])
    assert e_ref <= length / 10.0, (e_ref, length)
    assert abs(e_ref - O.E_REF) <= 1e-6, (e_ref, O.E_REF)               # (another libm may move the last digits, not the sixth)
    assert [s["passes"] for s in steps] == O.pass_schedule(cfg["n_scans"]) and all(s["status"] == 0 for s in steps)
    assert all(len(s["map_edge"]) > 10 and len(s["map_surf"]) > 50 for s in steps)
