"""The composition rule of the pair search's visible-chunk list (vis_composed_bound in csrc/iba_pair_plan.hpp through
iba_debug_vis_compose; no GPU): the entrywise bound, around the list's anchor, of every transform inside a group's own bound —
against a numpy restatement and against sampled transforms."""
import ctypes as C
import importlib

import numpy as np

pkg = importlib.import_module("spatial-temporal-lidar-camera-calibration_amd")
synth = importlib.import_module("spatial-temporal-lidar-camera-calibration_amd.synth")


def compose(Ra, ta, Rg, tg, rho_g, tau_g):
    L = pkg.load_library()
    out = np.zeros(12)
    args = [np.ascontiguousarray(a, np.float64).reshape(-1) for a in (Ra, ta, Rg, tg, rho_g, tau_g)]
    L.iba_debug_vis_compose.argtypes = [C.c_void_p] * 7
    st = L.iba_debug_vis_compose(*[a.ctypes.data_as(C.c_void_p) for a in args], out.ctypes.data_as(C.c_void_p))
    return st, out[:9].reshape(3, 3), out[9:]


def test_composed_bound_matches_numpy_and_covers_sampled_transforms():
    rng = np.random.default_rng(2)
    x0 = np.array([1.2, -1.2, 1.2, 0.0, -0.08, -0.27, 0.1])
    for _ in range(200):
        scale = 10.0 ** rng.uniform(-5, -1)
        xa, xg = synth.perturb(x0, rng, n=1)[0], synth.perturb(x0, rng, rot=scale, trans=10 * scale, n=1)[0]
        (Ra, ta, _), (Rg, tg, _) = synth.sim3_exp(xa), synth.sim3_exp(xg)
        rho_g, tau_g = rng.uniform(0, 3 * scale, (3, 3)), rng.uniform(0, 30 * scale, 3)
        st, rho, tau = compose(Ra, ta, Rg, tg, rho_g, tau_g)
        assert st == 0
        M, a = Rg @ Ra.T - np.eye(3), tg - Rg @ Ra.T @ ta
        rho_ref = np.abs(M) + rho_g @ (np.eye(3) + np.abs(M))
        tau_ref = np.abs(a) + rho_g @ np.abs(a) + tau_g
        # the library rounds up (1e-9 relative + 1e-15 on |M| and |a|, 1e-12 on the sums): never below the restatement, never far above
        assert np.all(rho >= rho_ref * (1 - 1e-13)) and np.all(rho <= rho_ref * (1 + 1e-8) + 1e-14)
        assert np.all(tau >= tau_ref * (1 - 1e-13)) and np.all(tau <= tau_ref * (1 + 1e-8) + 1e-14)
        # any transform inside the group's bound, T = (I + E) (R_g, t_g) + d with |E| <= rho_g, |d| <= tau_g, is inside the composed bound
        for _ in range(8):
            E, d = rng.uniform(-1, 1, (3, 3)) * rho_g, rng.uniform(-1, 1, 3) * tau_g
            Rt, tt = (np.eye(3) + E) @ Rg, (np.eye(3) + E) @ tg + d
            Mt, at = Rt @ Ra.T - np.eye(3), tt - Rt @ Ra.T @ ta
            assert np.all(np.abs(Mt) <= rho + 1e-15) and np.all(np.abs(at) <= tau + 1e-15)


def test_no_bound_for_a_nan_or_absurd_transform():
    I, z = np.eye(3), np.zeros(3)
    bad = I.copy(); bad[1, 1] = np.nan
    assert compose(I, z, bad, z, np.zeros((3, 3)), z)[0] != 0
    assert compose(I, z, I, np.array([0.0, np.inf, 0.0]), np.zeros((3, 3)), z)[0] != 0
    assert compose(I, z, I, z, np.full((3, 3), np.inf), z)[0] != 0
    st, rho, tau = compose(I, z, I, z, np.zeros((3, 3)), z)
    assert st == 0 and np.all(rho <= 1e-14) and np.all(tau <= 1e-14)


def covers(Ra, ta, rho_a, tau_a, Rg, tg, rho_g, tau_g):
    L = pkg.load_library()
    args = [np.ascontiguousarray(a, np.float64).reshape(-1) for a in (Ra, ta, rho_a, tau_a, Rg, tg, rho_g, tau_g)]
    L.iba_debug_vis_covers.argtypes = [C.c_void_p] * 8
    L.iba_debug_vis_covers.restype = C.c_int32
    return int(L.iba_debug_vis_covers(*[a.ctypes.data_as(C.c_void_p) for a in args]))


def test_covers_accepts_inside_rejects_outside_and_holds_at_the_corners():
    """vis_covers, the check a call makes before it walks the list: a group is accepted exactly when its composed bound fits entrywise; every
    CORNER transform of an accepted group (E = +-rho_g, d = +-tau_g, where the bound is tight) lies inside the anchor's bound"""
    rng = np.random.default_rng(6)
    x0 = np.array([1.2, -1.2, 1.2, 0.0, -0.08, -0.27, 0.1])
    n_in = n_out = 0
    for _ in range(300):
        scale = 10.0 ** rng.uniform(-4, -2)
        xa, xg = synth.perturb(x0, rng, n=1)[0], synth.perturb(x0, rng, rot=scale, trans=10 * scale, scale_rel=scale, n=1)[0]
        (Ra, ta, _), (Rg, tg, _) = synth.sim3_exp(xa), synth.sim3_exp(xg)
        rho_g, tau_g = rng.uniform(0, 3 * scale, (3, 3)), rng.uniform(0, 30 * scale, 3)
        st, rho, tau = compose(Ra, ta, Rg, tg, rho_g, tau_g)
        assert st == 0
        assert covers(Ra, ta, rho, tau, Rg, tg, rho_g, tau_g) == 1                      # the composed bound itself: accepted
        assert covers(Ra, ta, rho * 1.5 + 1e-6, tau * 1.5 + 1e-6, Rg, tg, rho_g, tau_g) == 1
        i, j = rng.integers(0, 3, 2)
        short_rho = rho.copy(); short_rho[i, j] *= 1 - 1e-6
        short_tau = tau.copy(); short_tau[i] *= 1 - 1e-6
        assert covers(Ra, ta, short_rho, tau, Rg, tg, rho_g, tau_g) == 0                 # one entry short: rejected
        assert covers(Ra, ta, rho, short_tau, Rg, tg, rho_g, tau_g) == 0
        # an anchor bound drawn at random: accepted exactly when the restated composition fits
        lo = 1.0 if rng.random() < 0.5 else 0.7
        rho_a, tau_a = rho * rng.uniform(lo, 1.6, (3, 3)), tau * rng.uniform(lo, 1.6, 3)
        want = bool(np.all(rho <= rho_a) and np.all(tau <= tau_a))
        assert covers(Ra, ta, rho_a, tau_a, Rg, tg, rho_g, tau_g) == int(want)
        n_in += want; n_out += not want
        for _ in range(8):   # corners of the group's bound
            E, d = rng.choice([-1.0, 1.0], (3, 3)) * rho_g, rng.choice([-1.0, 1.0], 3) * tau_g
            Rt, tt = (np.eye(3) + E) @ Rg, (np.eye(3) + E) @ tg + d
            Mt, at = Rt @ Ra.T - np.eye(3), tt - Rt @ Ra.T @ ta
            assert np.all(np.abs(Mt) <= rho + 1e-15) and np.all(np.abs(at) <= tau + 1e-15)
    assert n_out > 50 and n_in > 50
    nan = np.eye(3); nan[0, 0] = np.nan
    assert covers(np.eye(3), np.zeros(3), np.ones((3, 3)), np.ones(3), nan, np.zeros(3), np.zeros((3, 3)), np.zeros(3)) == 0


def culled(R, t, rho, tau, lo, hi, cam):
    L = pkg.load_library()
    g = np.concatenate([np.asarray(R, np.float64).reshape(-1), np.asarray(t, np.float64), np.asarray(rho, np.float64).reshape(-1), np.asarray(tau, np.float64)])
    box = np.array([lo[0], lo[1], lo[2], 0, hi[0], hi[1], hi[2], 0], np.float32)
    cam = np.asarray(cam, np.float64)
    L.iba_debug_chunk_box_culled.argtypes = [C.c_void_p] * 3
    L.iba_debug_chunk_box_culled.restype = C.c_int32
    return int(L.iba_debug_chunk_box_culled(g.ctypes.data_as(C.c_void_p), box.ctypes.data_as(C.c_void_p), cam.ctypes.data_as(C.c_void_p)))


def culled_np(R, t, rho, tau, lo, hi, cam):
    """chunk_box_culled restated (csrc/iba_split_kernels.hpp)"""
    fx, cx, cy, W, H = cam
    lo, hi = np.asarray(lo, np.float32).astype(np.float64), np.asarray(hi, np.float32).astype(np.float64)
    c, e = 0.5 * (lo + hi), 0.5 * (hi - lo)
    qc, ex = R @ c + t, np.abs(R) @ e
    a3 = np.abs(qc) + ex
    m = (ex + rho @ a3 + tau) * (1 + 1e-9) + 1e-9 * a3.sum() + 1e-9
    zhi = qc[2] + m[2]
    return bool(zhi <= 0 or fx * (qc[0] - m[0]) + (cx - W) * zhi >= 1e-6 * (fx * a3[0] + W * a3[2]) or fx * (qc[0] + m[0]) + cx * zhi < -1e-6 * (fx * a3[0] + W * a3[2])
                or fx * (qc[1] - m[1]) + (cy - H) * zhi >= 1e-6 * (fx * a3[1] + H * a3[2]) or fx * (qc[1] + m[1]) + cy * zhi < -1e-6 * (fx * a3[1] + H * a3[2]))


def test_what_the_list_culls_the_call_culls_too():
    """The list is built with the chunk test at the anchor and (1 + kappa) times the list's bound; a call inside the bound (vis_covers) runs the
    same test at its group's reference with the group's bound. Whatever the first culls the second must cull — on random boxes around the edge
    of the field of view, with the library's rebuild rule (composed bound x factor + floors of 1e-3 / 1e-2, caps 0.2 / 2) and its kappa
    (1e-3 max(1, W / min(cx, W - cx), H / min(cy, H - cy))). The function itself is checked against a numpy restatement on the way."""
    rng = np.random.default_rng(8)
    x0 = np.array([1.2, -1.2, 1.2, 0.0, -0.08, -0.27, 0.1])
    cams = ((718.856, 607.19, 185.22, 1241.0, 376.0), (700.0, 200.0, 300.0, 1000.0, 400.0))   # (the second: an off-centre principal point)
    n_cull_a = n_cull_g = n_mismatch = 0
    for it in range(400):
        cam = cams[it % 2]
        kappa = 1e-3 * max(1.0, cam[3] / min(cam[1], cam[3] - cam[1]), cam[4] / min(cam[2], cam[4] - cam[2]))
        scale = 10.0 ** rng.uniform(-5, -2.3)
        xa = synth.perturb(x0, rng, n=1)[0]
        Ra, ta, _ = synth.sim3_exp(xa)
        infl, rf, tf = rng.choice([1.0, 4.0, 16.0]), rng.choice([1e-3, 1e-2]), rng.choice([1e-2, 1e-1])
        # the group the list was built for, and the bound the list got
        rho_b, tau_b = rng.uniform(0, 3 * scale, (3, 3)), rng.uniform(0, 30 * scale, 3)
        st, rho0, tau0 = compose(Ra, ta, Ra, ta, rho_b, tau_b)
        rho_a, tau_a = rho0 * infl + rf, tau0 * infl + tf
        if rho_a.max() > 0.2 or tau_a.max() > 2.0:
            continue
        # a later call's group: somewhere inside the bound (shrunk until vis_covers accepts it), with a bound of its own
        for shrink in (1.0, 0.5, 0.25, 0.1, 0.0):
            xg = xa + shrink * rng.uniform(-1, 1, 7) * np.array([rho_a.max()] * 3 + [tau_a.max()] * 3 + [rho_a.max()]) * 0.7
            Rg, tg, _ = synth.sim3_exp(xg)
            rho_g, tau_g = shrink * rng.uniform(0, 0.3, (3, 3)) * rho_a, shrink * rng.uniform(0, 0.3, 3) * tau_a
            if covers(Ra, ta, rho_a, tau_a, Rg, tg, rho_g, tau_g) == 1:
                break
        else:
            raise AssertionError("the anchor's own reference must be covered")
        Rinv = np.linalg.inv(Ra)
        for _ in range(40):
            # a box placed in the anchor camera's frame near a border of the field of view (or behind the camera), mapped to the scanner's frame
            z = rng.choice([rng.uniform(0.5, 60.0), rng.uniform(-3.0, 0.5)])
            side = rng.integers(0, 4)
            u = (0.0, cam[3], rng.uniform(0, cam[3]), rng.uniform(0, cam[3]))[side] + rng.normal(0, 30.0)
            v = (rng.uniform(0, cam[4]), rng.uniform(0, cam[4]), 0.0, cam[4])[side] + rng.normal(0, 30.0)
            q = np.array([(u - cam[1]) / cam[0] * abs(z), (v - cam[2]) / cam[0] * abs(z), z])
            cpt = Rinv @ (q - ta)
            half = rng.uniform(0.01, 0.5, 3) * rng.choice([1.0, 0.05])
            lo, hi = cpt - half, cpt + half
            ca = culled(Ra, ta, rho_a * (1 + kappa), tau_a * (1 + kappa), lo, hi, cam)
            cg = culled(Rg, tg, rho_g, tau_g, lo, hi, cam)
            n_mismatch += (ca != culled_np(Ra, ta, rho_a * (1 + kappa), tau_a * (1 + kappa), lo, hi, cam)) + (cg != culled_np(Rg, tg, rho_g, tau_g, lo, hi, cam))
            assert not (ca == 1 and cg == 0), ("culled for the list, kept by the call", it, lo, hi)
            n_cull_a += ca; n_cull_g += cg
    assert n_cull_a > 1000 and n_cull_g > n_cull_a          # (the call's tighter bound culls more; both sides of the border were sampled)
    assert n_mismatch == 0
