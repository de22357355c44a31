"""Map-point refresh on the device (include/iba_mi355x.h, iba_refresh*): every output, count and kept stage of iba_refresh byte for byte against
tests/refresh_ref.py (S3 as the reference's sort and walk) AND against the host restatement (iba_debug_refresh_host), on the scenes of
tests/refresh_scene.py; tests/test_refresh_cpu.py asserts on the reference's output that every named case occurs in them. Then every narrow width
and both median forms, the whole hand scene on each wider shape, and the two chains: iba_triangulate -> refresh is R8's bytes, and iba_fuse ->
iba_fuse_apply -> iba_refresh_observations -> iba_refresh -> iba_refresh_store."""
import importlib

import numpy as np
import pytest

import refresh_ref as R
import refresh_scene as S

PKG = "spatial-temporal-lidar-camera-calibration_amd"
pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def rf():
    importlib.import_module(PKG)
    return importlib.import_module(PKG + ".refresh")


@pytest.fixture(scope="module")
def mm():
    return importlib.import_module(PKG + ".map_match")


@pytest.fixture(scope="module")
def om():
    return importlib.import_module(PKG + ".orb_match")


@pytest.fixture(scope="module")
def scenes():
    out = {}
    for name, make in (("hand", S.hand_scene), ("random", S.random_scene)):
        sc = make()
        out[name] = (sc, R.run(sc))
    return out


def expected_paths(sc, ref, narrow=16, min_path=0):
    """the points each device shape takes: by the length of the FULL list, never below min_path"""
    n_obs = np.diff(sc["obs_off"])[ref["point"]][ref["status"] == R.REFRESHED]
    path = np.maximum(np.where(n_obs <= narrow, 0, np.where(n_obs <= 64, 1, 2)), min_path)
    return np.bincount(path, minlength=3).astype(np.int32)


@pytest.mark.parametrize("name", ["hand", "random"])
def test_device_against_ref_and_host(rf, mm, om, scenes, name):
    sc, ref = scenes[name]
    n_obs = np.diff(sc["obs_off"])[ref["point"]]
    if name == "hand":
        assert set(S.COUNTS) <= set(n_obs.tolist()) and all(c > 0 for c in ref["counts"]["geo_state"]) and all(c > 0 for c in ref["counts"]["desc_state"])
    else:
        assert len(ref["point"]) == 207 and n_obs.max() > 64 and all(c > 0 for c in ref["counts"]["status"])
    args = S.lib_args(rf, mm, om, sc)
    dev = rf.refresh(*args, keep_stages=1)
    S.assert_equal(dev, ref)
    paths = dev.counts()["path"]
    assert S.same_bytes(paths, expected_paths(sc, ref)) and all(p > 0 for p in paths)
    host = rf.refresh_host(*args, keep_stages=1)
    S.same_results(dev, host)
    host.close()
    dev.close()
    plain = rf.refresh(*args)                          # without keep_stages: the same results
    S.assert_equal(plain, ref, keep_stages=False)
    plain.close()


@pytest.mark.parametrize("median", [0, 1])
@pytest.mark.parametrize("lanes", [4, 8, 16, 32])
def test_narrow_widths_and_median_forms_give_the_same_bytes(rf, mm, om, scenes, monkeypatch, lanes, median):
    monkeypatch.setenv("IBA_DEBUG_ENV", "1")
    monkeypatch.setenv("IBA_REFRESH_NARROW_LANES", str(lanes))
    monkeypatch.setenv("IBA_REFRESH_MEDIAN", str(median))
    for name in ("hand", "random"):
        sc, ref = scenes[name]
        dev = rf.refresh(*S.lib_args(rf, mm, om, sc), keep_stages=1)
        S.assert_equal(dev, ref)
        assert S.same_bytes(dev.counts()["path"], expected_paths(sc, ref, narrow=lanes))
        dev.close()


@pytest.mark.parametrize("median", [0, 1])
@pytest.mark.parametrize("min_path", [1, 2])
def test_whole_hand_scene_on_each_wider_shape(rf, mm, om, scenes, monkeypatch, min_path, median):
    monkeypatch.setenv("IBA_DEBUG_ENV", "1")
    monkeypatch.setenv("IBA_REFRESH_MIN_PATH", str(min_path))
    monkeypatch.setenv("IBA_REFRESH_MEDIAN", str(median))
    sc, ref = scenes["hand"]
    dev = rf.refresh(*S.lib_args(rf, mm, om, sc), keep_stages=1)
    S.assert_equal(dev, ref)
    paths = dev.counts()["path"]
    assert S.same_bytes(paths, expected_paths(sc, ref, min_path=min_path)) and not paths[:min_path].any()
    dev.close()


def test_triangulate_chain(rf, mm, om):
    S.check_triangulate_chain(rf, mm, om, importlib.import_module(PKG + ".triangulate"), host=False)


def test_fuse_chain(rf, mm, om):
    S.check_fuse_chain(rf, importlib.import_module(PKG + ".fuse"), mm, om, host=False)
