"""ORB extraction on the device (include/iba_mi355x.h, iba_orb_*): every stage and every output BYTE FOR BYTE against the numpy restatement
tests/orb_ref.py, with keep_stages = 1 so that a mismatch names its stage: pyramid levels, score maps, candidates, blurred levels, keypoints, angles,
responses, octaves, sizes, descriptors and all counts. Images are the seeded mosaics of tests/orb_scene.py."""
import importlib
import math

import numpy as np
import pytest

import orb_ref as R
import orb_scene as S

PKG = "spatial-temporal-lidar-camera-calibration_amd"
pytestmark = pytest.mark.gpu
F = np.float32
RAGGED = ((97, 83, 1), (200, 150, 2), (320, 120, 3))


@pytest.fixture(scope="module")
def orb():
    importlib.import_module(PKG)
    return importlib.import_module(PKG + ".orb")


@pytest.fixture(scope="module")
def pat():
    return S.pattern()


@pytest.fixture(scope="module")
def images():
    imgs = [S.image(W, H, seed) for W, H, seed in RAGGED]
    imgs[1] = S.strided(imgs[1])      # stride > W
    assert imgs[1].strides[0] > imgs[1].shape[1]
    return imgs


_ref_cache = {}


def ref_of(img, pat, **opts):
    key = (img.tobytes(), img.shape, tuple(sorted(opts.items())), pat.tobytes())
    if key not in _ref_cache:
        _ref_cache[key] = R.extract(np.ascontiguousarray(img), pat, **opts)
    return _ref_cache[key]


def bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


def compare(f, i, r, n_levels, stages=True):
    """image i of the result f against the reference r: 0 differing bytes, stage by stage"""
    c = f.counts(i)
    assert c["candidates_per_level"].tolist() == r["candidates_per_level"], "candidate counts"
    assert c["fallback_cells_per_level"].tolist() == r["fallback_cells_per_level"], "fallback cells"
    if stages:
        for l in range(n_levels):
            wh = r["plan"]["level_wh"][l]
            assert np.array_equal(f.level(i, l, wh), r["levels"][l]), "pyramid level %d" % l
            assert np.array_equal(f.scores(i, l, wh), r["scores"][l]), "score map %d" % l
            xy, sc = f.candidates(i, l)
            assert np.array_equal(xy, r["cand_xy"][l]) and np.array_equal(sc, r["cand_score"][l]), "candidates %d" % l
    assert c["per_level"].tolist() == r["per_level"] and c["n_keypoints"] == r["n_keypoints"], "keypoint counts"
    if stages:
        for l in range(n_levels):
            assert np.array_equal(f.level(i, l, r["plan"]["level_wh"][l], blurred=True), r["blurred"][l]), "blurred level %d" % l
    k = f.read(i)
    for name in ("octave", "xy", "response", "size", "angle", "desc"):
        assert np.array_equal(bits(k[name]), bits(r[name])), name
    return c["n_keypoints"]


def test_ragged_batch(orb, pat, images):
    f = orb.extract(images, pattern=pat, n_features=300, keep_stages=1)
    assert len(f) == 3
    total = sum(compare(f, i, ref_of(images[i], pat, n_features=300), 8) for i in range(3))
    assert total > 300
    f.close()


def test_small_n_features(orb, pat, images):
    refs = [ref_of(im, pat, n_features=60) for im in images]
    st = [r["stats"] for r in refs]
    assert any(s["phase2"] for s in st) and any(s["size_tie"] for s in st)
    assert sum(s["fallback_cells"] for s in st) > 0 and sum(s["suppression_ties"] for s in st) > 0
    f = orb.extract(images, pattern=pat, n_features=60, keep_stages=1)
    for i in range(3):
        compare(f, i, refs[i], 8)
    f.close()


@pytest.mark.parametrize("opts", [dict(n_levels=1, n_features=200), dict(n_levels=3, scale_factor=2.0, n_features=200)])
def test_level_shapes(orb, pat, images, opts):
    f = orb.extract(images[1:], pattern=pat, keep_stages=1, **opts)
    for i in range(2):
        assert compare(f, i, ref_of(images[1 + i], pat, **opts), opts["n_levels"]) > 0
    f.close()


def test_flat_image(orb, pat):
    flat = np.full((90, 140), 77, np.uint8)
    f = orb.extract([flat], pattern=pat, keep_stages=1)
    r = ref_of(flat, pat)
    assert r["n_keypoints"] == 0 and sum(r["fallback_cells_per_level"]) > 0
    assert compare(f, 0, r, 8) == 0
    k = f.read(0)
    assert k["xy"].shape == (0, 2) and k["desc"].shape == (0, 32)
    f.close()


def test_equal_thresholds(orb, pat, images):
    opts = dict(ini_th_fast=12, min_th_fast=12, n_features=150)
    f = orb.extract(images[:2], pattern=pat, keep_stages=1, **opts)
    for i in range(2):
        compare(f, i, ref_of(images[i], pat, **opts), 8)
    f.close()


def _tie_angles():
    """float32 angles whose rounded cosine or sine times 18 is exactly k + 0.5: O9's rint meets a tie at an axis point of radius 18"""
    out = []
    for k in range(18):
        for base in (math.degrees(math.acos((k + 0.5) / 18.0)), math.degrees(math.asin((k + 0.5) / 18.0))):
            lo = hi = F(base)
            cands = [lo]
            for _ in range(400):
                lo, hi = np.nextafter(lo, F(-np.inf)), np.nextafter(hi, F(np.inf))
                cands += [lo, hi]
            cands = np.array(cands, F)
            a, b = R.angle_ab(cands)
            pa, pb = (F(18) * a).astype(F), (F(18) * b).astype(F)
            hit = (np.abs(pa - np.trunc(pa)) == 0.5) | (np.abs(pb - np.trunc(pb)) == 0.5)
            out += cands[hit][:2].tolist()
    return np.array(out, F)


def test_rint_ties_in_the_descriptor(orb):
    angles = _tie_angles()
    assert len(angles) >= 8
    angles = np.concatenate([angles, F([0, 90, 180, 270, 360, 33.3])])
    axis = np.array([[18, 0, 0, 18], [-18, 0, 0, -18], [18, 0, -18, 0], [0, 18, 0, -18]], np.int8)
    tie_pat = np.tile(axis, (64, 1))
    img = S.image(121, 103, 9)
    rng = np.random.default_rng(11)
    xy = np.stack([rng.integers(19, 121 - 19, len(angles)), rng.integers(19, 103 - 19, len(angles))], axis=1).astype(np.int32)
    xy[0], xy[1] = (19, 19), (121 - 20, 103 - 20)      # the nearest a keypoint comes to the edge
    blurred, desc = orb.describe(img, xy, angles, tie_pat)
    want_blur = R.blur(img)
    assert np.array_equal(blurred, want_blur)
    stats = {}
    want = np.array([R.describe(want_blur, int(x), int(y), a, tie_pat, stats) for (x, y), a in zip(xy, angles)], np.uint8)
    assert stats["rint_ties"] >= 8
    assert np.array_equal(desc, want)


def test_batch_independence(orb, pat, images, monkeypatch):
    def everything(f, i):
        k = f.read(i)
        c = f.counts(i)
        return b"".join(bits(k[n]).tobytes() for n in ("xy", "angle", "response", "octave", "size", "desc")) + b"".join(
            bits(c[n]).tobytes() for n in ("per_level", "candidates_per_level", "fallback_cells_per_level"))
    batch = orb.extract(images, pattern=pat, n_features=300)
    assert batch.n_chunks == 1
    whole = [everything(batch, i) for i in range(3)]
    again = orb.extract(images, pattern=pat, n_features=300)
    assert [everything(again, i) for i in range(3)] == whole        # two runs, the same bytes
    for i in range(3):
        alone = orb.extract([images[i]], pattern=pat, n_features=300)
        assert everything(alone, 0) == whole[i]
        alone.close()
    monkeypatch.setenv("IBA_ORB_BUDGET", "1")                        # less than one image: a chunk still holds one
    cut = orb.extract(images, pattern=pat, n_features=300, keep_stages=1)
    monkeypatch.delenv("IBA_ORB_BUDGET")
    assert cut.n_chunks == 3
    assert [everything(cut, i) for i in range(3)] == whole
    compare(cut, 2, ref_of(images[2], pat, n_features=300), 8)      # the stage accessors reach the right chunk
    for f in (batch, again, cut):
        f.close()


def test_errors_touch_no_device(orb, pat, images):
    err = importlib.import_module(PKG).IbaError
    bad = pat.copy()
    bad[0] = [13, 13, 0, 0]
    for call in (lambda: orb.extract([], pattern=pat), lambda: orb.extract(images), lambda: orb.extract(images, pattern=bad),
                 lambda: orb.extract(images, pattern=pat, n_levels=17), lambda: orb.extract(images, pattern=pat, min_th_fast=30),
                 lambda: orb.extract(images + [S.image(100, 260, 4)], pattern=pat)):
        with pytest.raises(err) as e:
            call()
        assert e.value.status == 1
    f = orb.extract(images[:1], pattern=pat)
    for call in (lambda: f.counts(1), lambda: f.read(-1), lambda: f.level(0, 0, (97, 83)), lambda: f.scores(0, 0, (97, 83)), lambda: f.candidates(0, 0)):
        with pytest.raises(err) as e:
            call()
        assert e.value.status == 1
    f.close()
