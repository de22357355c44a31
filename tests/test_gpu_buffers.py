"""Ownership of device memory (csrc/iba_device_buf.hpp): every buffer belongs to the object or scope that declares it, so closing an object and
leaving an entry point, by an error return as well, give back what they allocated. The tests only count bytes: free device memory as hipMemGetInfo
reports it (torch.cuda.mem_get_info) after a synchronise, before and after many repetitions. Nothing here provokes an allocation failure.
Bounds (conditions, not measurements; the drifts measured are in profiles/buffers_parity.md):
  life cycle    20 cycles of create / use / close drift by less than the footprint of ONE handle, taken inside the test (twenty leaked handles
                would be twenty times it)
  error return  64 refused calls of iba_floam_extract drift by less than 8 x 16 x N bytes: by the time rule 3 refuses the scan, its scan, block,
                count and four sort buffers are allocated (at least 16 B per point), so leaking those alone would cost 64 x 16 x N."""
import importlib

import numpy as np
import pytest

import ba_scene
import floam_ref as F
import pgo_ref as R

pytestmark = pytest.mark.gpu
PKG = "spatial-temporal-lidar-camera-calibration_amd"


def _free():
    import torch
    torch.cuda.synchronize()
    return int(torch.cuda.mem_get_info()[0])     # hipMemGetInfo


def test_twenty_life_cycles_of_every_owner_give_their_memory_back(pkg, abi, synth):
    ba = importlib.import_module(PKG + ".ba")
    pgo = importlib.import_module(PKG + ".pgo")
    prob, meta = synth.make_scene(n_frames=4, pts_per_frame=3000)
    prm = abi.reference_yaml_params()
    xs = synth.perturb(meta["x_gt"], np.random.default_rng(0), n=4)
    src = np.asarray(prob.frame_points(1), np.float64)
    g = R.case_graph(16, seed=3)
    ba_prob, _ = ba_scene.make(n_frames=5, pts_per_frame=50, seed=2, ba=ba)
    footprint = []

    def cycle():
        before = _free()
        h = pkg.IbaHandle(prob, prm)
        footprint.append(before - _free())
        h.eval_cost(xs)
        h.eval_normal(xs)
        h.icp_register(src, np.eye(4))
        h.scan_step([(1, 0, np.eye(4))], 1.0)
        h.submap_build([([0, 1], [np.eye(4), np.eye(4)], None, 0.5)])
        h.floam_extract([0])
        h.debug_nn(0, src[:100])
        db = h.sc_describe([0, 1, 2, 3])
        pg = pgo.PoseGraph(g.nodes, g.edge_tuples())
        bh = ba.BaHandle(ba_prob)
        bh.close()
        pg.close()
        db.close()
        h.close()

    cycle()                                       # code objects, rocPRIM, the runtime's pools
    free0 = _free()
    for _ in range(20):
        cycle()
    free1 = _free()
    one = min(footprint[1:])
    print("buffers-figures life-cycle: footprint of one handle", one, "B; drift over 20 cycles", free0 - free1, "B")
    assert one > 0 and free0 - free1 < one


def test_sixty_four_refused_extractions_leave_free_memory_where_it_was(pkg, abi):
    ring = 41
    scan = F.ring_scan(64, {ring: 60000}, seed=4)    # one elevation: every point falls in one ring, far above IBA_FLOAM_MAX_RING_POINTS
    N = len(scan)
    assert N == 60000 and F.MAX_RING_POINTS == 8192
    h = pkg.IbaHandle(abi.Problem.from_scans([scan]), abi.reference_yaml_params(0))
    message = ("IBA_ERR_UNSUPPORTED: iba_floam_extract: scan 0 (frame 0), ring %d holds %d points; a ring list holds at most 8192 (IBA_FLOAM_MAX_RING_POINTS)" % (ring, N))

    def refused():
        with pytest.raises(pkg.IbaError) as ex:
            h.floam_extract([0])
        assert ex.value.status == 4 and str(ex.value) == message, (ex.value.status, str(ex.value))

    refused()
    free0 = _free()
    for _ in range(64):
        refused()
    free1 = _free()
    h.close()
    print("buffers-figures error-return: N", N, "drift over 64 refused calls", free0 - free1, "B; bound", 8 * 16 * N, "B")
    assert free0 - free1 < 8 * 16 * N
