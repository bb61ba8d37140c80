"""The interior body of the streaming reduce kernel (k_stack_reduce3, csrc/sg_stack.hip: SUM /
MAX / MIN / MEAN NO_REJEC, src/stacking/stacking.c:196-355, 824-1128, 1786-1794) against the
oracle, bit for bit.

A wave segment of 128 SEG pixels is interior when no shifted column can leave the image
(`x0 > max|shiftx| && x0 + 128 SEG + max|shiftx| <= W`); it then takes the fast body: one SGPR
offset per frame from the shift table, dword loads at 2-byte alignment, rows shifted out of the
frame reading 0 from the buffer bounds check (a negative start included), two register buffers
with a straight-line steady loop and a three-way tail, packed u16 MAX / MIN, MIN's per-frame
shifty test, XCD-aware dealing of the workgroups.  The other reduce tests are too narrow to
have an interior segment (tests/test_gpu_edges.py, test_gpu_bands.py: W <= 200), so every test
here asserts through `interior_segments` that its shape has interior AND edge segments.

Data: uniform u16 in [1, 65535] with a few planted 0 and 65535, so a MIN that takes the zero
fill of a row shifted out of its frame as a candidate turns most of the image to 0 (the
oracle's MIN image is asserted to be under 1 % zeros).  Frame 0 is unshifted (from 3 frames
on; with 2 frames they carry +max and -max), the x shifts always hold +max|shiftx| and
-max|shiftx|, the y shifts a frame at +9, one at -9 and one wholly out of the frame (H + 3);
SUM / MAX / MIN also take +30, -30 and -(H + 2).  MEAN keeps negative y shifts below the
reference's block height (H / 4 with one thread, stacking.c:1560; the oracle returns -4 beyond
it and the library refuses).  No tolerances: every comparison is exact.
"""
import functools

import numpy as np
import pytest

import oracle_lib as orc
import sirilgpu as sg
from test_gpu_bands import _dev, _stack_bands
from test_gpu_edges import _with_env
from test_gpu_stack import assert_same, gpu_stack

pytestmark = pytest.mark.gpu

KINDS = ["sum", "max", "min", "mean", "mean-additive", "mean-multiplicative"]
METHOD = {"sum": sg.SUM, "max": sg.MAX, "min": sg.MIN, "mean": sg.MEAN, "mean-additive": sg.MEAN,
          "mean-multiplicative": sg.MEAN}
NORM = {"mean-additive": sg.ADDITIVE_SCALING, "mean-multiplicative": sg.MULTIPLICATIVE_SCALING}


def MEAN_Y(H):
    return [H + 3, 9, -9]                       # accepted by the reference's block reads at H >= 40


def EXTREME_Y(H):
    return [30, -(H + 2), -30, H + 3, 9, -9]    # SUM / MAX / MIN: any row shift


def BAND_Y(H):
    return [9, -9]


def interior_segments(W, maxsx, seg=1):
    """k_stack_reduce3<M, seg>'s segment starts of one row: (interior, edge).  A workgroup is 4
    waves of 128 seg pixels; a segment at x0 is interior when x0 > maxsx and
    x0 + 128 seg + maxsx <= W; the other segments that hold a pixel take the per-lane loop"""
    pxw = 128 * seg
    starts = range(0, -(-W // (4 * pxw)) * 4 * pxw, pxw)
    inner = [x0 for x0 in starts if x0 > maxsx and x0 + pxw + maxsx <= W]
    edge = [x0 for x0 in starts if x0 < W and x0 not in inner]
    return inner, edge


def _premise(W, sx, seg=1):
    """the shape runs both bodies; fails loudly if a change moves it onto the edge path only"""
    maxsx = 0 if sx is None else int(np.abs(sx).max())
    inner, edge = interior_segments(W, maxsx, seg)
    assert inner, f"W={W} max|shiftx|={maxsx} SEG={seg}: no interior segment, the fast body would not run"
    assert edge, f"W={W} max|shiftx|={maxsx} SEG={seg}: no edge segment"
    return inner, edge


def test_interior_segments_counts():
    """the restated predicate at the shapes below (counted by hand from the kernel's constants)"""
    assert [len(interior_segments(1101, 16, s)[0]) for s in (1, 2, 4)] == [7, 3, 1]
    assert [len(interior_segments(400, 16, s)[0]) for s in (1, 2, 4)] == [2, 0, 0]
    assert interior_segments(200, 16)[0] == []             # the older reduce tests' widest image
    assert interior_segments(1101, 16)[0] == list(range(128, 1024, 128))
    assert interior_segments(1101, 16)[1] == [0, 1024]


@functools.lru_cache(maxsize=None)
def _pool(C, H, W, nmax):
    """nmax frames of the shape; tests take the first N (read only)"""
    rng = np.random.default_rng(1000003 * C + 1009 * H + W)
    frames = rng.integers(1, 65536, size=(nmax, C, H, W)).astype(np.uint16)
    flat = frames.reshape(-1)
    at = rng.choice(flat.size, size=2 * max(4, nmax // 2), replace=False)
    flat[at[0::2]] = 0
    flat[at[1::2]] = 65535
    return frames


def _frames(N, C, H, W):
    nmax = 33 if C > 1 else 130 if W == 1101 else 48
    assert N <= nmax
    return _pool(C, H, W, nmax)[:N]


def _shifts(N, H, maxsx, yplants, seed):
    rng = np.random.default_rng(seed)
    sx = rng.integers(-maxsx, maxsx + 1, N).astype(np.int32)
    sy = rng.integers(-9, 10, N).astype(np.int32)
    sx[0] = sy[0] = 0
    if N == 2:
        sx[:] = [maxsx, -maxsx]
    else:
        sx[1], sx[N - 1] = maxsx, -maxsx
    # the planted row shifts on frames spread over 1 .. N - 1, the last one (-9) on the last frame
    plants = yplants(H)[-(N - 1):]
    k = len(plants)
    for i, v in enumerate(plants):
        sy[N - 1 if k == 1 else 1 + i * (N - 2) // (k - 1)] = v
    assert sx.max() == maxsx and sx.min() == -maxsx and all(v in sy for v in plants)
    return sx, sy


def _case(kind, N, C, H, W, maxsx=16, shifts=True, yplants=None):
    """(frames, sx, sy, normalisation kwargs) of a kind at a shape"""
    frames = _frames(N, C, H, W)
    sx = sy = None
    if shifts:
        if yplants is None:
            yplants = MEAN_Y if METHOD[kind] == sg.MEAN else EXTREME_Y
        sx, sy = _shifts(N, H, maxsx, yplants, 7 * N + W + maxsx)
    kw = {}
    if kind in NORM:
        rng = np.random.default_rng(77 + W + N + NORM[kind])
        kw = dict(normalize=NORM[kind], offset=rng.uniform(-300, 300, N), mul=rng.uniform(0.8, 1.2, N),
                  scale=rng.uniform(0.9, 1.1, N))
    return frames, sx, sy, kw


def _oracle(kind, frames, sx, sy, kw):
    """(image, SUM's maximum or None)"""
    if kind == "sum":
        rc, ref, mref = orc.stack_sum(frames, sx, sy)
        assert rc == 0 and mref > 65535, (rc, mref)         # the 65535 / max scaling branch (:328-342)
        return ref, mref
    if kind in ("max", "min"):
        rc, ref = orc.stack_maxmin(frames, kind == "max", sx, sy)
        assert rc == 0
        if kind == "min":
            # the premise of the data: a zero-filled row counted as a candidate would show
            assert np.count_nonzero(ref == 0) < 0.01 * ref.size, np.count_nonzero(ref == 0)
        return ref, None
    rc, ref, _ = orc.stack_rejection(frames, sg.NO_REJEC, shiftx=sx, shifty=sy, max_thread=1, **kw)
    assert rc == 0, "the reference's block reads refuse these shifts"
    return ref, None


def _gpu(ctx, kind, frames, sx, sy, kw):
    out, _, maxim = gpu_stack(ctx, frames, METHOD[kind], shiftx=sx, shifty=sy, max_thread=1, **kw)
    return out, maxim


def _gpu_device(ctx, kind, frames, sx, sy, kw):
    """one sg_stack_u16_device call over every row: (image, maximum, the main kernel's blocks)"""
    import torch
    N, C, H, W = frames.shape
    d_in = _dev(frames)
    d_out = torch.zeros(C * H * W, dtype=torch.int16, device="cuda")
    torch.cuda.synchronize()
    desc, keep = sg.make_desc(METHOD[kind], N, W, H, C, shiftx=sx, shifty=sy, max_thread=1, max_number_of_rows=H,
                              **kw)
    _, maxim = ctx.stack_device(desc, d_in.data_ptr(), C * H * W, H * W, d_out.data_ptr(), 0, H)
    torch.cuda.synchronize()
    return d_out.cpu().numpy().view(np.uint16).reshape(C, H, W), maxim, ctx.stats().main_kernel_blocks


def _check(out, maxim, ref, mref, what):
    assert_same(out, ref, what)
    if mref is not None:
        assert maxim == mref, (what, maxim, mref)


def _blocks3(W, H, C, seg=1):
    return -(-W // (512 * seg)) * H * C


@pytest.mark.parametrize("N", [2, 15, 16, 17, 31, 32, 33, 47, 48, 49, 64, 65, 97, 130])
@pytest.mark.parametrize("kind", KINDS)
def test_interior_methods_frame_counts(gpu_ctx, kind, N):
    """every method at frame counts that end in one, two and three tail blocks, each full and
    partial (N % 16 != 0: `full` false, frames past N load nothing), with the steady loop not
    entered, entered once and several times, and MIN's shifty reload at frame 64; odd W, so
    every second row starts on a 2-byte boundary before any shift"""
    H, W = 40, 1101
    frames, sx, sy, kw = _case(kind, N, 1, H, W)
    _premise(W, sx)
    ref, mref = _oracle(kind, frames, sx, sy, kw)
    out, maxim = _gpu(gpu_ctx, kind, frames, sx, sy, kw)
    _check(out, maxim, ref, mref, f"{kind} N={N}")


@pytest.mark.parametrize("N", [17, 48])
@pytest.mark.parametrize("W,maxsx", [(400, 16), (1101, 127)])
@pytest.mark.parametrize("kind", KINDS)
def test_interior_predicate_boundaries(gpu_ctx, kind, W, maxsx, N):
    """both ends of the interior predicate met with equality: at W = 400 the last interior
    segment ends at x0 + 128 + 16 == W (its last lane's pair reads columns W - 2 and W - 1 of the
    frame shifted by -16); at max|shiftx| = 127 segment 128 is interior (x0 == max + 1) and its
    first lane reads column 1 of the frame shifted by +127"""
    H = 40
    frames, sx, sy, kw = _case(kind, N, 1, H, W, maxsx=maxsx)
    inner, edge = _premise(W, sx)
    if W == 400:
        assert inner[-1] + 128 + maxsx == W and len(inner) == 2
    else:
        assert inner[0] == maxsx + 1 == 128 and inner[0] - int(sx.max()) == 1
    ref, mref = _oracle(kind, frames, sx, sy, kw)
    out, maxim = _gpu(gpu_ctx, kind, frames, sx, sy, kw)
    _check(out, maxim, ref, mref, f"{kind} W={W} max|sx|={maxsx} N={N}")


@pytest.mark.parametrize("shifts", [True, False])
@pytest.mark.parametrize("N", [16, 33])
@pytest.mark.parametrize("H", [40, 41])
@pytest.mark.parametrize("kind", KINDS)
def test_interior_planes_and_no_shifts(gpu_ctx, kind, H, N, shifts):
    """three planes in one launch (`rr % nrows`, `rr / nrows`, the plane stride), with shifts and
    without (use_shift false: max|shiftx| 0 and a zero table; segment 0 stays on the edge loop).
    The workgroups are dealt over the 8 XCDs: 3 x 40 x 3 = 360 is a multiple of 8 (`rem` == 0),
    3 x 41 x 3 = 369 is not (`rem` == 1), and the grid shows k_stack_reduce3 ran"""
    C, W = 3, 1101
    frames, sx, sy, kw = _case(kind, N, C, H, W, shifts=shifts)
    inner, _ = _premise(W, sx)
    assert inner == list(range(128, 1024, 128))
    ref, mref = _oracle(kind, frames, sx, sy, kw)
    out, maxim, blocks = _gpu_device(gpu_ctx, kind, frames, sx, sy, kw)
    assert blocks == _blocks3(W, H, C) and (blocks % 8 == 0) == (H == 40), blocks
    _check(out, maxim, ref, mref, f"{kind} C=3 H={H} N={N} shifts={shifts}")


@pytest.mark.parametrize("seg", [1, 2, 4])
def test_interior_seg_grid(gpu_ctx, seg):
    """k_stack_reduce3<M, SEG> really runs under SG_REDUCE_SEG: its grid is ceil(W / (512 SEG))
    workgroups per row and plane (the other two reduce kernels have grids of their own), on one
    device-path call per SEG"""
    N, C, H, W = 17, 2, 40, 1101
    for kind in ("mean", "min"):
        frames, sx, sy, kw = _case(kind, N, C, H, W)
        _premise(W, sx, seg)
        ref, mref = _oracle(kind, frames, sx, sy, kw)
        out, maxim, blocks = _with_env("SG_REDUCE_SEG", str(seg),
                                       lambda c: _gpu_device(c, kind, frames, sx, sy, kw))
        assert blocks == _blocks3(W, H, C, seg), (seg, blocks)
        _check(out, maxim, ref, mref, f"{kind} SEG={seg}")


@pytest.mark.parametrize("seg", [2, 4])
@pytest.mark.parametrize("kind", KINDS)
def test_interior_seg_2_and_4(gpu_ctx, kind, seg):
    """the SG_REDUCE_SEG=2 / 4 instantiations (register buffers of 8 / 4 frames, 2 / 4 dwords per
    lane and frame): frame counts around one, two and three of their blocks and into the steady
    loop"""
    H, W = 40, 1101

    def run(ctx):
        for N in (2, 7, 9, 12, 13, 24, 25, 70):
            frames, sx, sy, kw = _case(kind, N, 1, H, W)
            _premise(W, sx, seg)
            ref, mref = _oracle(kind, frames, sx, sy, kw)
            out, maxim = _gpu(ctx, kind, frames, sx, sy, kw)
            _check(out, maxim, ref, mref, f"{kind} SEG={seg} N={N}")

    _with_env("SG_REDUCE_SEG", str(seg), run)


@pytest.mark.parametrize("N", [17, 65])
@pytest.mark.parametrize("kind", KINDS)
def test_interior_equals_other_reduce_kernels(gpu_ctx, kind, N):
    """the default kernel's image equals the one-pixel-per-lane kernel's (SG_REDUCE1=1,
    k_stack_reduce) and the per-lane pair kernel's on its own launch shape (SG_REDUCE1=2,
    k_stack_reduce2); each grid shows which kernel ran"""
    C, H, W = 1, 40, 1101
    frames, sx, sy, kw = _case(kind, N, C, H, W)
    _premise(W, sx)
    ref, mref = _oracle(kind, frames, sx, sy, kw)
    out, maxim, blocks = _gpu_device(gpu_ctx, kind, frames, sx, sy, kw)
    assert blocks == _blocks3(W, H, C), blocks
    _check(out, maxim, ref, mref, f"{kind} N={N}")
    for knob, grid_x in (("1", -(-W // 256)), ("2", -(-((W + 1) // 2) // 256))):
        o, m, b = _with_env("SG_REDUCE1", knob, lambda c: _gpu_device(c, kind, frames, sx, sy, kw))
        assert b == grid_x * H * C, (knob, b)
        assert_same(out, o, f"{kind} N={N}: default vs SG_REDUCE1={knob}")
        assert m == maxim, (knob, m, maxim)


@pytest.mark.parametrize("kind", KINDS)
def test_reduce2_route_without_knob(gpu_ctx, kind):
    """one frame shifted by 20000 columns: the shift table's 16-bit forms do not hold it
    (hist_addr_ok false), so the call takes k_stack_reduce2 on its own grid with no knob set;
    that frame contributes nothing to any pixel"""
    N, C, H, W = 17, 1, 40, 1101
    frames, sx, sy, kw = _case(kind, N, C, H, W)
    sx = sx.copy()
    sx[5] = 20000
    ref, mref = _oracle(kind, frames, sx, sy, kw)
    out, maxim, blocks = _gpu_device(gpu_ctx, kind, frames, sx, sy, kw)
    assert blocks == -(-((W + 1) // 2) // 256) * H * C, blocks
    _check(out, maxim, ref, mref, f"{kind} shiftx=20000")


@pytest.mark.parametrize("resident", ["full", "band"])
@pytest.mark.parametrize("kind", ["mean", "max", "min"])
def test_interior_row_bands(gpu_ctx, kind, resident):
    """three row bands, each one device call (row_begin > 0; with only the band and its shift
    halo resident, a biased base pointer): two planes, rows shifted out above the first band and
    below the last; the bands together equal the oracle's whole image"""
    N, C, H, W = 33, 2, 40, 1101
    frames, sx, sy, kw = _case(kind, N, C, H, W, yplants=BAND_Y)
    assert np.abs(sy).max() == 9
    _premise(W, sx)
    ref, _ = _oracle(kind, frames, sx, sy, kw)
    out, _ = _stack_bands(gpu_ctx, frames, METHOD[kind], sg.NO_REJEC, (4.0, 3.0), sx, sy, 1, 3, resident)
    assert_same(out, ref, f"bands {kind} resident={resident}")
