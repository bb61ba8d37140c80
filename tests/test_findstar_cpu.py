"""tests/findstar_ref.py against itself, without a GPU: the literal and the vectorised forms agree,
pass 1 of the smooth is exact, the hand-checked cases of peaker's threshold and peak test, and every
"distinguishing" condition tests/test_gpu_findstar.py relies on for the seeds it uses (a wrong
filter order, a wrong tie rule, an unordered or uncapped list, a re-associated sigma would each
change what is compared there)."""
import numpy as np
import pytest

import findstar_ref as fr
from prepro_ref import mean_sigma_u16


@pytest.mark.parametrize("H,W", [(32, 32), (33, 37), (40, 48)])
def test_smooth_literal_equals_vectorised(H, W):
    img = fr.noise_frame(100 + W, H, W).astype(np.float32)
    p1l, p1v = fr.smooth_literal(img, 1), fr.smooth(img, 1)
    assert p1l.tobytes() == p1v.tobytes()
    p2l, p2v = fr.smooth_literal(p1l, 2), fr.smooth(p1v, 2)
    assert p2l.tobytes() == p2v.tobytes()
    assert p2v.tobytes() == fr.float_plane(img.astype(np.uint16)).tobytes()


@pytest.mark.parametrize("H,W", [(32, 32), (33, 37), (40, 48)])
def test_pass1_is_exact(H, W):
    img = fr.noise_frame(200 + W, H, W)
    p1 = fr.smooth(img.astype(np.float32), 1)
    exact = fr.smooth_exact(img, 1)          # multiples of 1/256 below 2^16: exact in float64 and float32
    assert np.array_equal(p1.astype(np.float64), exact)
    assert np.array_equal(exact * 256, np.rint(exact * 256))


def test_plane_never_exceeds_65535():
    """reget_rawdata's ratio: float adds, double products and sums and the final rounding are all
    monotone, and the all-65535 image gives exactly 65535, so no input passes it; near-saturated
    frames stay at or below it"""
    sat = np.full((40, 48), 65535, dtype=np.uint16)
    assert (fr.float_plane(sat) == np.float32(65535)).all()
    rng = np.random.default_rng(0)
    for _ in range(20):
        img = rng.integers(65000, 65536, size=(40, 48)).astype(np.uint16)
        img[rng.random(img.shape) < 0.7] = 65535
        assert fr.float_plane(img).max() <= np.float32(65535)
        assert fr.detection_plane(img)[2] == 0


# ------------------------------------------------------------------ what the GPU tests rely on

@pytest.mark.parametrize("H,W", fr.PLANE_SHAPES)
def test_separable_variant_differs(H, W):
    img = fr.plane_case(H, W)
    a, b = fr.detection_plane(img)[0], fr.detection_plane(img, fr.smooth_separable)[0]
    assert (a != b).any()
    assert (fr.float_plane(img) != fr.float_plane(img, fr.smooth_separable)).sum() > a.size // 20


def test_tie_image_hits_every_branch():
    img = fr.tie_image()
    rec = fr.threshold(img, 1.0)
    assert rec["median"] == 10.0 and 10 < rec["threshold"] < min(fr.TIE_VALUES) and not rec["wrapped"]
    wave, applied, _ = fr.detection_plane(img)
    assert applied == 0 and np.array_equal(wave, img)
    ref = fr.peaks(wave, rec["threshold"], 1)
    assert ref == fr.peaks_literal(wave, rec["threshold"], 1) and len(ref) > 50
    assert fr.peaks(wave, rec["threshold"], 1, rule="gt_only") != ref
    assert fr.peaks(wave, rec["threshold"], 1, rule="ge_all") != ref
    # for each of the eight positions: a pixel above the threshold without a greater neighbour whose
    # only equal neighbour sits there, so that position alone decides it
    top = img[::-1].astype(np.int64)
    c = top[1:-1, 1:-1]
    nbs = {(dy, dx): top[1 + dy:top.shape[0] - 1 + dy, 1 + dx:top.shape[1] - 1 + dx]
           for dy in (-1, 0, 1) for dx in (-1, 0, 1) if (dy, dx) != (0, 0)}
    no_greater = np.all([nb <= c for nb in nbs.values()], axis=0) & (c > rec["threshold"])
    for pos, nb in nbs.items():
        others_less = np.all([o < c for q, o in nbs.items() if q != pos], axis=0)
        assert (no_greater & (nb == c) & others_less).any(), pos


def test_noise_frame_rules_and_prefix():
    img = fr.noise_frame(64, 64, 64)
    ref, rec, wave = fr.candidates(img, 0.0, 2)
    assert len(ref) > 10 and ref == fr.peaks_literal(wave, rec["threshold"], 2)
    assert ref == sorted(ref, key=lambda c: (c[1], c[0]))           # raster order
    assert len({c[1] for c in ref}) > 3                             # over several rows
    # capped: a strict prefix, and not what a scan in another order would keep first
    assert 10 < len(ref) and ref[:10] != sorted(ref)[:10]


def test_star_fields_have_candidates():
    for i in range(len(fr.STAR_CASES)):
        img, r = fr.star_case(i)
        ref, rec, wave = fr.candidates(img, 1.0, r)
        assert len(ref) >= 2 and not rec["wrapped"], (img.shape, len(ref))
        assert ref == fr.peaks_literal(wave, rec["threshold"], r)
        assert fr.threshold(img, 100.0)["wrapped"] == 1


def test_bright_frame_sigma_depends_on_order():
    img = fr.bright_frame()
    exact, s2 = fr.sigma_from_sums(img)
    assert s2 >= 2 ** 53
    _, _, seq = mean_sigma_u16(img)
    assert np.float64(seq).tobytes() != np.float64(exact).tobytes()
    small = fr.noise_frame(1, 40, 48)
    assert np.float64(mean_sigma_u16(small)[2]).tobytes() == np.float64(fr.sigma_from_sums(small)[0]).tobytes()


# ------------------------------------------------------------------ hand-checked cases

def test_single_bright_pixel():
    img = np.full((31, 40), 100, dtype=np.uint16)
    img[31 - 1 - 12, 17] = 30000                                    # display (17, 12)
    cands, rec, wave = fr.candidates(img, 1.0, 3)
    assert rec["median"] == 100.0 and rec["ngood"] == 31 * 40 and np.array_equal(wave, img)
    assert cands == [(17, 12)]
    box = fr.boxes(img, cands, 3)[0]
    assert box[3, 3] == 30000 and box.sum() == 30000 + 35 * 100     # z(r, r) is the candidate


def test_threshold_and_norm_bounds():
    img = np.full((31, 64), 50, dtype=np.uint16)
    for x, v in [(5, 65535), (15, 65534), (25, 7000), (35, 7001)]:
        img[10, x] = v
    top_y = 31 - 1 - 10
    assert fr.peaks(img, 7000, 2) == [(15, top_y), (35, top_y)]     # == threshold and == norm are out
    assert fr.peaks_literal(img, 7000, 2) == [(15, top_y), (35, top_y)]


def test_plateau_keeps_its_first_pixel():
    """:192-196 rejects a pixel with an equal neighbour in the row above or to its left, so of a
    2x2 equal plateau the pixel first met in raster order (top-left on the display) survives"""
    img = np.full((31, 40), 20, dtype=np.uint16)
    top = img[::-1]
    top[8:10, 20:22] = 9000
    for f in (fr.peaks, fr.peaks_literal):
        assert f(img, 100, 2) == [(20, 8)]
    assert fr.peaks(img, 100, 2, rule="gt_only") == [(20, 8), (21, 8), (20, 9), (21, 9)]
    assert fr.peaks(img, 100, 2, rule="ge_all") == []


def test_half_saturated_median_is_zero():
    img = np.full((10, 10), 65535, dtype=np.uint16)
    img[:4] = 300
    rec = fr.threshold(img, 1.0)
    assert rec["ngood"] == 100 and rec["median"] == 0.0 and not rec["no_data"]
    assert rec["threshold"] == fr.to_word(1.0 * fr.to_word(rec["sigma"]))


def test_single_nonzero_pixel_sigma_zero():
    img = np.zeros((8, 8), dtype=np.uint16)
    img[3, 3] = 777
    rec = fr.threshold(img, 5.0)
    assert rec["ngood"] == 1 and rec["sigma"] == 0.0 and rec["median"] == 777.0 and rec["threshold"] == 777
    assert fr.threshold(np.zeros((8, 8), dtype=np.uint16), 1.0)["no_data"] == 1


def test_word_conversion():
    assert fr.to_word(65535.9) == 65535 and fr.to_word(65536.0) == 0 and fr.to_word(65537.5) == 1
    assert fr.to_word(2147483647.5) == 0xFFFF and fr.to_word(2147483648.0) == 0 and fr.to_word(float("nan")) == 0
    assert fr.to_word(1e300) == 0
