"""The SIGMA finish of the histogram kernel (sgh_sigma3 in csrc/sg_stack_hist.hip) at the inputs where
its threshold conversions, its rounding-band test and its moment products have an edge.

Every case stacks 4 rows of 512 pixels without shifts (sixteen 128-pixel tiles: the image's edge
tiles and interior ones; the reference's block partition takes no image of fewer than 4 rows),
SIGMA through PATH_AUTO (the histogram kernel), and compares the image and both rejection counters
exactly with the C oracle and with PATH_SORTED.  A build that sent every pixel to the redo list
would pass such a comparison, so each case but the sigma = 0 one also bounds slow_pixels +
chain_pixels (the redo list) by 2 % of its pixels.  Measured on an MI355X before the finish was
changed and after, the same: clamp edges 0 of 2048 pixels at both sigma pairs, each side 0, large
moments 13; with bright columns spread over 65300..65534 the clamp case had 244 (12 %): the band's
last start is 65279, and where the median of a column's first 16 frames fell below 65407 its
samples near 65534 lay above the band.

  clamp edges    N = 40: dark columns (0..40 and one or two 65535s: blo - tol < 0) and bright ones
                 (65420..65534 and one or two zeros: bhi + tol > 65535); sig (4, 3) and (40, 30), where
                 the thresholds lie tens of thousands outside [0, 65535] and the conversion's
                 saturation and the integer clamp do the clamping
  sigma = 0      N = 200 (below the u8 bin limit): constant columns, two-valued ones, constant but
                 for one sample (exact0, tol = 0, num <= 0)
  each side      N = 64, round(normal(1000, 30)) kept within 100 of 1000 (the band is 256 bins around
                 the median of 16 frames): 1 or 2 zeros only, 1 or 2 65535s only, or both: the
                 low-only, high-only and two-sided removals, odd and even kept counts
  large moments  N = 512: 190..210 zeros beside samples near 60000: the largest n SS - S^2 terms of
                 this frame count
"""
import functools

import numpy as np
import pytest

import oracle_lib as orc
import sirilgpu as sg
from test_gpu_stack import assert_same

pytestmark = pytest.mark.gpu

H, W = 4, 512
REDO_SHARE = 0.02


def _scatter(rng, col, values):
    """put `values` at random frames of the column (in place)"""
    at = rng.permutation(len(col))[:len(values)]
    col[at] = values


@functools.lru_cache(maxsize=None)
def _frames(case):
    """[N][1][H][W] frames of a case (read only); column x of row r is of kind (x + r) % kinds"""
    rng = np.random.default_rng({"clamp": 40, "sigma0": 200, "sides": 64, "moments": 512}[case])
    N = {"clamp": 40, "sigma0": 200, "sides": 64, "moments": 512}[case]
    f = np.zeros((N, 1, H, W), np.uint16)
    for r in range(H):
        for x in range(W):
            k = x + r
            if case == "clamp":
                if k % 2 == 0:
                    col = rng.integers(0, 41, size=N)
                    _scatter(rng, col, [65535] * (1 + (k // 2) % 2))
                else:
                    col = rng.integers(65420, 65535, size=N)
                    _scatter(rng, col, [0] * (1 + (k // 2) % 2))
            elif case == "sigma0":
                c = int(rng.integers(500, 60000))
                col = np.full(N, c)
                if k % 4 == 1:      # two values, d apart, in any proportion
                    col[rng.permutation(N)[:int(rng.integers(1, N))]] = c + int(rng.integers(1, 60))
                elif k % 4 == 2:    # one sample off, inside the band
                    _scatter(rng, col, [c + int(rng.choice([-40, -1, 1, 40]))])
                elif k % 4 == 3:    # one sample off, at 0 or 65535
                    _scatter(rng, col, [int(rng.choice([0, 65535]))])
            elif case == "sides":
                col = np.clip(np.rint(rng.normal(1000.0, 30.0, size=N)), 900, 1100).astype(np.int64)
                _scatter(rng, col, [[0], [0, 0], [65535], [65535, 65535], [0, 65535], [0, 0, 65535, 65535]][k % 6])
            else:
                col = np.clip(np.rint(rng.normal(60000.0, 30.0, size=N)), 59900, 60100).astype(np.int64)
                _scatter(rng, col, [0] * int(rng.integers(190, 211)))
            f[:, 0, r, x] = col
    f.setflags(write=False)
    return f


@functools.lru_cache(maxsize=None)
def _oracle(case, sig):
    rc, ref, rej = orc.stack_rejection(_frames(case), sg.SIGMA, sig=sig, max_thread=1)
    assert rc == 0
    return ref, rej


def _gpu(ctx, case, sig, path):
    frames = _frames(case)
    N = frames.shape[0]
    desc, keep = sg.make_desc(sg.MEAN, N, W, H, 1, rejection=sg.SIGMA, sig=sig, max_thread=1, max_number_of_rows=H,
                              kernel_path=path)
    rc, out, rej, _ = ctx.stack_host(desc, frames)
    assert rc == 0, ctx.error()
    return out, rej, ctx.stats()


def _check(ctx, case, sig, bound_redo=True):
    ref, rej_ref = _oracle(case, sig)
    out, rej, st = _gpu(ctx, case, sig, sg.PATH_AUTO)
    redo = int(st.slow_pixels) + int(st.chain_pixels)
    print(f"{case} sig={sig}: path={st.path} slow_pixels={st.slow_pixels} chain_pixels={st.chain_pixels} "
          f"of {H * W} rej={rej[0].tolist()}")
    assert st.path == 1
    assert_same(out, ref, f"{case} {sig} histogram path")
    assert np.array_equal(rej, rej_ref), (rej, rej_ref)
    srt, rej_s, st_s = _gpu(ctx, case, sig, sg.PATH_SORTED)
    assert st_s.path == 0
    assert_same(out, srt, f"{case} {sig} histogram path against the sorted path")
    assert np.array_equal(rej, rej_s), (rej, rej_s)
    if bound_redo:
        assert redo <= REDO_SHARE * H * W, (redo, H * W)


@pytest.mark.parametrize("sig", [(4.0, 3.0), (40.0, 30.0)])
def test_clamp_edges(gpu_ctx, sig):
    _check(gpu_ctx, "clamp", sig)


def test_sigma_zero_and_near_it(gpu_ctx):
    _check(gpu_ctx, "sigma0", (4.0, 3.0), bound_redo=False)


def test_each_side_alone(gpu_ctx):
    _check(gpu_ctx, "sides", (4.0, 3.0))


def test_large_moments(gpu_ctx):
    _check(gpu_ctx, "moments", (4.0, 3.0))
