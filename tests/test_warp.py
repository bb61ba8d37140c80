"""Perspective warp (a17, sg_warp.hip) vs the numpy restatement of OpenCV's warpPerspective
(tests/warp_ref.py) and hand-derived known answers (identity, integer translations,
rotations by 90 and 180 degrees, mirrors, a half-pixel linear shift).  Parity with a real
OpenCV build is unpinned (OpenCV absent, version unpinned)."""
import numpy as np
import pytest

import sirilgpu as sg
import warp_ref


def _img(C, H, W, seed):
    rng = np.random.default_rng(seed)
    img = (1000 + rng.integers(0, 3000, size=(C, H, W))).astype(np.uint16)
    img[:, H // 3, W // 4] = 65535
    return img


def test_reference_known_answers():
    img = _img(1, 9, 11, 1)
    for interp in (0, 1, 3, 4):
        assert np.array_equal(warp_ref.warp(img, np.eye(3), interp=interp), img)
    # display-coordinate translation by (+2, +1): out(x, y) = in(x - 2, y - 1), 0 outside
    Hm = np.array([[1, 0, 2], [0, 1, 1], [0, 0, 1]], dtype=np.float64)
    disp = img[:, ::-1, :]
    exp = np.zeros_like(disp)
    exp[:, 1:, 2:] = disp[:, :-1, :-2]
    for interp in (0, 1, 3, 4):
        assert np.array_equal(warp_ref.warp(img, Hm, interp=interp), exp[:, ::-1, :]), interp


@pytest.mark.gpu
@pytest.mark.parametrize("interp", [0, 1, 2, 3, 4])
@pytest.mark.parametrize("C", [1, 3])
def test_warp_matches_reference(gpu_ctx, interp, C):
    rng = np.random.default_rng(10 + interp + C)
    H, W = 57, 83
    img = _img(C, H, W, interp)
    for k in range(3):
        a = rng.normal(0, 0.05)
        Hm = np.array([[np.cos(a), -np.sin(a), rng.normal(0, 4)],
                       [np.sin(a), np.cos(a), rng.normal(0, 4)],
                       [rng.normal(0, 2e-4), rng.normal(0, 2e-4), 1.0]])
        out_size = (W, H) if k < 2 else (W + 9, H - 5)
        got = gpu_ctx.warp(img, Hm, out_size, interp)
        exp = warp_ref.warp(img, Hm, out_size, interp)
        assert np.array_equal(got, exp), (interp, C, k, np.argwhere(got != exp)[:5])


@pytest.mark.gpu
def test_warp_identity_and_translation(gpu_ctx):
    img = _img(3, 40, 70, 3)
    Hm = np.array([[1, 0, -3], [0, 1, 5], [0, 0, 1]], dtype=np.float64)
    for interp in (0, 1, 3, 4):
        assert np.array_equal(gpu_ctx.warp(img, np.eye(3), None, interp), img)
        assert np.array_equal(gpu_ctx.warp(img, Hm, None, interp), warp_ref.warp(img, Hm, None, interp))


# ---- shapes and homographies the near-identity cases above never reach ----

INTERPS = (0, 1, 3, 4)


def _feat(C, H=23, W=31, seed=0):
    """random 1000..3999 with a 4 x 4 plateau of 65535, a 2 x 4 block of zeros and 65535 at
    the four corners: both ends of saturate_cast<ushort> lie next to ordinary values"""
    rng = np.random.default_rng(100 + seed)
    img = (1000 + rng.integers(0, 3000, size=(C, H, W))).astype(np.uint16)
    if H >= 16 and W >= 16:
        img[:, 5:9, 6:10] = 65535
        img[:, 14:16, 20:24] = 0
    img[:, ::H - 1 if H > 1 else 1, ::W - 1 if W > 1 else 1] = 65535
    return img


def _known_answers(img):
    """[(name, hom, out_size, interpolations, expected)] derived by hand, in memory order.
    Display row y is memory row H-1-y; a map that is symmetric under the row flip has the
    same form in both."""
    C, H, W = img.shape
    cases = []
    # (x, y) -> (W-1-x, H-1-y): all coordinates are integers, so every interpolation's
    # weights are (.., 1, ..) on the pixel itself
    cases.append(("rot180", [[-1, 0, W - 1], [0, -1, H - 1], [0, 0, 1]], None, INTERPS, img[:, ::-1, ::-1]))
    cases.append(("mirror", [[-1, 0, W - 1], [0, 1, 0], [0, 0, 1]], None, INTERPS, img[:, :, ::-1]))
    # (x, y) -> (H-1-y, x) into an H-wide, W-high output: out_disp[y', x'] = in_disp[H-1-x', y'],
    # in_disp = img[::-1], so out_disp = img.T and the memory image is img.T flipped
    cases.append(("rot90", [[0, -1, H - 1], [1, 0, 0], [0, 0, 1]], (H, W), INTERPS,
                  np.transpose(img, (0, 2, 1))[:, ::-1, :]))
    # x -> x + 0.5: destination x reads source x - 0.5, i.e. cvRound(32 (x - 0.5)) = 32 (x - 1) + 16:
    # pixels x-1 and x with the weights (0.5, 0.5), exact in float32, then rint (half to
    # even).  Pixel x-1 is outside for x = 0, so the border's 0 enters on the LEFT: column 0
    # is rint(img[0] / 2) and the source's last column only ever counts half, in column W-1.
    a = np.concatenate([np.zeros((C, H, 1)), img[:, :, :-1].astype(np.float64)], axis=2)
    half = np.rint((a + img.astype(np.float64)) / 2).astype(np.uint16)
    cases.append(("half_pixel", [[1, 0, 0.5], [0, 1, 0], [0, 0, 1]], None, (1, 2), half))
    return cases


KNOWN = ["rot180", "mirror", "rot90", "half_pixel"]


def _known(name, C):
    return next(k for k in _known_answers(_feat(C, seed=C)) if k[0] == name)


@pytest.mark.parametrize("name", KNOWN)
def test_reference_rotations_mirror_half_pixel(name):
    """the hand-derived answers hold for the restatement itself"""
    for C in (1, 3):
        _, hom, out_size, interps, exp = _known(name, C)
        for interp in interps:
            assert np.array_equal(warp_ref.warp(_feat(C, seed=C), hom, out_size, interp), exp), (C, interp)


def test_reference_options_change_nothing_by_default():
    img = _feat(1, 9, 300, seed=5)
    hom = [[1, 0, -0.3], [0, 1, 0.2], [1e-4, 0, 1]]
    for interp in INTERPS:
        a = warp_ref.warp(img, hom, None, interp)
        b, sums = warp_ref.warp(img, hom, None, interp, bw=113, return_sums=True)   # 113 is what 9 rows give
        assert np.array_equal(a, b)
        assert np.array_equal(np.clip(np.rint(sums), 0, 65535).astype(np.uint16), a)


@pytest.mark.gpu
@pytest.mark.parametrize("name", KNOWN)
def test_warp_known_answers(gpu_ctx, name):
    for C in (1, 3):
        _, hom, out_size, interps, exp = _known(name, C)
        for interp in interps:
            got = gpu_ctx.warp(_feat(C, seed=C), hom, out_size, interp)
            assert np.array_equal(got, exp), (C, interp, np.argwhere(got != exp)[:5])


def _rot(a, tx, ty):
    return [[np.cos(a), -np.sin(a), tx], [np.sin(a), np.cos(a), ty], [0, 0, 1]]


HOMOGRAPHIES = {
    # name: (hom, out_size (width, height) or None)
    "zoom_into_5_rows": ([[2.3, 0, 0], [0, 2.3, 0], [0, 0, 1]], (70, 5)),     # 5 rows: bw = 70, not 64
    "shrink": ([[0.37, 0, 0], [0, 0.41, 0], [0, 0, 1]], None),
    "w_crosses_zero": ([[1, 0, 0], [0, 1, 0], [0.05, 0.02, 1]], None),      # W = 1 - 0.05 x - 0.02 y
    "w_grows": ([[1, 0, 0], [0, 1, 0], [-0.1, 0, 1]], None),
    "singular": ([[1, 2, 3], [2, 4, 6], [0, 0, 1]], None),
}


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(HOMOGRAPHIES))
def test_warp_homographies(gpu_ctx, name):
    hom, out_size = HOMOGRAPHIES[name]
    for C in (1, 3):
        img = _feat(C, seed=10 + C)
        for interp in INTERPS:
            exp = warp_ref.warp(img, hom, out_size, interp)
            if name == "singular":      # cv::invert leaves M = 0: X = Y = 0, source display pixel (0, 0)
                assert np.array_equal(exp, np.broadcast_to(img[:, -1:, :1], exp.shape))
            if name == "w_crosses_zero":
                assert exp.any() and not exp.all()
            got = gpu_ctx.warp(img, hom, out_size, interp)
            assert np.array_equal(got, exp), (C, interp, np.argwhere(got != exp)[:5])


@pytest.mark.gpu
@pytest.mark.parametrize("t", [1e7, -1e7, 1e9, -1e9])
def test_warp_far_translation_is_zero(gpu_ctx, t):
    """the coordinates saturate the short range (1e7) and the int range before it (32e9 > 2^31)"""
    hom = [[1, 0, t], [0, 1, -t], [0, 0, 1]]
    for C in (1, 3):
        img = _feat(C, seed=20 + C)
        for interp in INTERPS:
            assert not warp_ref.warp(img, hom, None, interp).any()
            assert not gpu_ctx.warp(img, hom, None, interp).any(), (C, interp)


@pytest.mark.gpu
@pytest.mark.parametrize("interp", [3, 4])
def test_warp_saturates_both_ends(gpu_ctx, interp):
    """negative cubic / Lanczos lobes next to the 65535 plateau and the zero block: the float
    sums leave [0, 65535] on both sides and saturate_cast<ushort> clamps them"""
    hom = [[1, 0, 0.5], [0, 1, 0], [0, 0, 1]]
    for C in (1, 3):
        img = _feat(C, seed=30 + C)
        exp, sums = warp_ref.warp(img, hom, None, interp, return_sums=True)
        assert sums.min() < -0.5 and sums.max() > 65535.5, (sums.min(), sums.max())
        assert (exp[sums < -0.5] == 0).all() and (exp[sums > 65535.5] == 65535).all()
        got = gpu_ctx.warp(img, hom, None, interp)
        assert np.array_equal(got, exp), (C, np.argwhere(got != exp)[:5])


@pytest.mark.gpu
@pytest.mark.parametrize("H,W", [(1, 1), (3, 5), (8, 8)])
def test_warp_small_sources(gpu_ctx, H, W):
    """sources below the cubic (4) and Lanczos (8) supports: 1 x 1; 3 x 5, all border branch;
    8 x 8, where the identity has exactly one interior Lanczos position (3, 3)"""
    for C in (1, 3):
        img = _feat(C, H, W, seed=40 + C)
        for interp in INTERPS:
            got = gpu_ctx.warp(img, np.eye(3), None, interp)
            assert np.array_equal(got, img), (C, interp)
            hom = _rot(0.1, 0.3, -0.2)
            exp = warp_ref.warp(img, hom, None, interp)
            got = gpu_ctx.warp(img, hom, None, interp)
            assert np.array_equal(got, exp), (C, interp, np.argwhere(got != exp)[:5])


@pytest.mark.gpu
@pytest.mark.parametrize("interp", [0, 1])
def test_warp_block_association(gpu_ctx, interp):
    """9 output rows: OpenCV's column blocks are 1024 / 9 = 113 wide, not the kernel's 64-wide
    x tiles.  X = (M0 xb + M2) + M0 (x - xb) is rounded per block, and the translation puts
    every X within a few ulps of a rounding tie (nearest: x + 0.5; linear: 32 X = .. + 0.5),
    so the block origin xb decides which way hundreds of pixels fall."""
    t = (0.5 if interp == 0 else 0.5 / 32) + 9 * 2.0 ** -49
    hom = [[1, 0, -t], [0, 1, 0], [0, 0, 1]]
    for C in (1, 3):
        img = np.random.default_rng(50 + C).integers(1000, 60000, size=(C, 9, 300)).astype(np.uint16)
        exp = warp_ref.warp(img, hom, None, interp)
        assert np.array_equal(exp, warp_ref.warp(img, hom, None, interp, bw=113))
        other = warp_ref.warp(img, hom, None, interp, bw=64)
        assert (exp != other).sum() >= 100 * C, (exp != other).sum()       # else the case proves nothing
        got = gpu_ctx.warp(img, hom, None, interp)
        assert np.array_equal(got, exp), (C, (got != exp).sum(), (got != other).sum())
