"""Rejection, median and sum stacks at the frame counts above 512 where the plan
(siril-0.9_amd/csrc/sg_stack_plan.hpp) or a kernel changes code, against the C oracle, bit for bit:
the image, the rejection counters, SUM's maximum, and through sg_stack_stats the route taken.

  512 | 513     pick_nreg 8 -> 16 (k_stack_sorted<16, *>), k_stack_replay<512> -> <2048>, LINEARFIT KM 8 -> 16
  1024 | 1025   no sorted kernel: the redo list goes to the literal kernel, `compact` off
  1448 | 1449   histogram WINSORIZED: double moments -> 64-bit integer moments (SGH_WIN_DBL_MAXN)
  2048 | 2049   no replay kernel (SG_REPLAY_MAXN)
  3276 | 3277   the literal kernel's thread count leaves SG_LIT_THREADS (1 GiB of scratch)
  ~ 2896        n SS - S^2 of a column of counted zeros / 65535s passes 2^53 (sgh_sigma_fast)
  65535 | 65536 histogram path -> every pixel to the literal kernel
  65537 | 65538 SUM / MEAN without rejection: N 65535 passes 2^32 - 1 (SG_SUM_U32_MAXN)

The frames of the rejection tests (`_columns`) are noise the histogram kernel decides itself plus
marked pixel columns (all zero, saturated, constant, half dark / half bright, counted extremes, far
outliers); the CPU tests at the end prove the properties of those inputs the GPU tests lean on.
"""
import functools
import warnings

import numpy as np
import pytest

import oracle_lib as orc
import sirilgpu as sg
from test_gpu_stack import assert_same

gpu = pytest.mark.gpu

SIG = {"sigma": (3.0, 3.0), "winsorized": (3.0, 3.0), "percentile": (0.2, 0.1), "sigmedian": (3.0, 3.0),
       "linearfit": (3.0, 3.0), "median": (0.0, 0.0)}
REJ = {"sigma": sg.SIGMA, "winsorized": sg.WINSORIZED, "percentile": sg.PERCENTILE, "sigmedian": sg.SIGMEDIAN,
       "linearfit": sg.LINEARFIT, "median": sg.NO_REJEC}

HIST_COUNTS = [513, 1024, 1025, 1448, 1449, 2047, 2049, 3277, 4099]
HIST_CASES = [(N, k) for N in HIST_COUNTS for k in ("sigma", "winsorized")] + \
             [(N, k) for N in (513, 1024, 1025, 4099) for k in ("percentile", "sigmedian", "median")]
RUN_LEN = 4                                             # pixels of a marked run


def _geom(N):
    """(H, max_thread, maxshift): 4 reference blocks of 4 rows with |shifty| < 4 up to 2049 frames,
    of 2 rows with |shifty| < 2 above (the oracle's CPU time)"""
    return (16, 2, 3) if N <= 2049 else (8, 1, 1)


def _run_starts(W):
    """first pixel of the 9 marked runs: from column 0 (the edge tile, columns a shift empties) to
    W - RUN_LEN (the partial last tile), the middle ones in between"""
    return [round(i * (W - RUN_LEN) / 8) for i in range(9)]


@functools.lru_cache(maxsize=3)
def _columns(N, H, W, seed):
    """(frames [N][1][H][W], marked [H][W]) of a mono sequence (read only).  Background
    round(normal(1000, 20)); on row H // 2 nine runs of RUN_LEN marked pixel columns: all zero, all
    65535, constant 1500 (u8 bin overflow), half dark / half bright (a random half of the frames 0,
    the rest round(normal(60000, 20))), counted extremes (k in 1, 2, 5, N // 8 samples at 0 and as
    many at 65535) and 0.2 % far outliers in 20000..60000 (at least one per column).  `marked` also
    holds the few background columns with a sample further than 100 from the median of their first
    16 frames (a 5 sigma tail: a handful among 8 M samples), so every unmarked column lies inside
    the histogram kernel's 256-bin band around that median."""
    rng = np.random.default_rng(seed)
    f = np.rint(rng.normal(1000.0, 20.0, size=(N, 1, H, W))).astype(np.uint16)
    marked = np.zeros((H, W), bool)
    r = H // 2
    xs = _run_starts(W)
    span = [slice(x, x + RUN_LEN) for x in xs]
    f[:, 0, r, span[0]] = 0
    f[:, 0, r, span[1]] = 65535
    f[:, 0, r, span[2]] = 1500
    for x in range(xs[3], xs[3] + RUN_LEN):
        f[:, 0, r, x] = np.rint(rng.normal(60000.0, 20.0, size=N))
        f[rng.permutation(N)[: N // 2], 0, r, x] = 0
    for s, k in zip(span[4:8], (1, 2, 5, N // 8)):
        for x in range(s.start, s.stop):
            at = rng.permutation(N)[: 2 * k]
            f[at[:k], 0, r, x] = 0
            f[at[k:], 0, r, x] = 65535
    for x in range(xs[8], xs[8] + RUN_LEN):
        m = rng.random(N) < 0.002
        m[rng.integers(N)] = True
        f[m, 0, r, x] = rng.integers(20000, 60000, size=int(m.sum()))
    for s in span:
        marked[r, s] = True
    centre = np.median(f[:16, 0].astype(np.int32), axis=0)
    far = (np.abs(f[:, 0].astype(np.int32) - centre) > 100).any(axis=0)
    marked |= far
    f.setflags(write=False)
    return f, marked


def _touched(marked, sx, sy):
    """output pixels whose stack holds a sample of a marked column, or lies on a row that a frame's
    shift empties (R - shifty outside the frame: zero fill)"""
    H, W = marked.shape
    out = np.zeros((H, W), bool)
    for dx, dy in set(zip(sx.tolist(), sy.tolist())):
        R, X = np.arange(H) - dy, np.arange(W) - dx
        rok, xok = (R >= 0) & (R < H), (X >= 0) & (X < W)
        out[~rok, :] = True
        sub = marked[np.ix_(R[rok], X[xok])]
        out[np.ix_(np.nonzero(rok)[0], np.nonzero(xok)[0])] |= sub
    return out


def _coeffs(normalize, N, seed):
    """the reference's coefficients for frames measured as they are: location 1000 and one common
    scale, with a frame-to-frame jitter of 0.4 % and 1 %, so a normalised noise column moves by some
    15 levels and stays inside the histogram band"""
    rng = np.random.default_rng(seed)
    loc = 1000 + rng.random(N) * 4
    scl = 30 + rng.random(N) * 0.3
    return orc.compute_normalization(normalize, loc, scl, ref_image=0)


TRIO_X = 140                                            # between two marked runs, in the interior tile


def _captured_trio(frames, sx, sy):
    """a copy of the frames with RUN_LEN columns the normalised histogram kernel captures whole and
    still cannot decide: three out-of-band samples (690 and 845 below the band, 5000 above it), in
    three unshifted frames so that the output pixels hold all three.  The sample at 5000 raises the
    first pass's sigma to about 127 at 1024 frames, so the SIGMA threshold (3 sigma: 619) and
    Winsorize's first clamp (1.5 sigma: 809) fall below the captured 845, where the kernel does not
    count: the pixel leaves for the compact list (up to 1024 frames) or the redo list (beyond)"""
    still = np.nonzero((sx == 0) & (sy == 0))[0]
    assert len(still) >= 3
    f = frames.copy()
    r = f.shape[2] // 2
    for k, v in zip(still[:3], (690, 845, 5000)):
        f[k, 0, r, TRIO_X:TRIO_X + RUN_LEN] = v
    return f


def _stack_both(ctx, frames, kind, sx, sy, max_thread, normalize=sg.NO_NORM, coeffs=(None, None, None),
                kernel_path=sg.PATH_AUTO):
    """the oracle and the GPU (host-pull path) on the same frames: (ref, rej_ref, out, rej, stats)"""
    N, C, H, W = frames.shape
    off, mul, sc = coeffs
    if kind == "median":
        rc, ref = orc.stack_median(frames, normalize, off, mul, sc, max_thread=max_thread)
        rej_ref = np.zeros((3, 2), np.uint64)
        sx = sy = None
    else:
        rc, ref, rej_ref = orc.stack_rejection(frames, REJ[kind], sig=SIG[kind], shiftx=sx, shifty=sy,
                                               normalize=normalize, offset=off, mul=mul, scale=sc,
                                               max_thread=max_thread)
    assert rc == 0
    desc, keep = sg.make_desc(sg.MEDIAN if kind == "median" else sg.MEAN, N, W, H, C, rejection=REJ[kind],
                              normalize=normalize, sig=SIG[kind], shiftx=sx, shifty=sy, offset=off, mul=mul, scale=sc,
                              max_thread=max_thread, max_number_of_rows=H, kernel_path=kernel_path)
    rc, out, rej, _ = ctx.stack_host(desc, frames)
    assert rc == 0, ctx.error()
    return ref, rej_ref, out, rej, ctx.stats()


_hist_runs = {}


def _hist_run(ctx, N, kind):
    """one PATH_AUTO stack per case, shared by the parity and the fast-path tests"""
    if (N, kind) not in _hist_runs:
        H, mt, ms = _geom(N)
        frames, marked = _columns(N, H, 260, N)
        sx, sy = orc.synth_shifts(N, seed=N, maxshift=ms)
        ref, rej_ref, out, rej, st = _stack_both(ctx, frames, kind, sx, sy, mt)
        _hist_runs[(N, kind)] = dict(ref=ref, rej_ref=rej_ref, out=out, rej=rej, path=st.path,
                                     chain_pixels=int(st.chain_pixels), touched=_touched(marked, sx, sy))
    return _hist_runs[(N, kind)]


@gpu
@pytest.mark.parametrize("N,kind", HIST_CASES)
def test_hist_route_across_counts(gpu_ctx, N, kind):
    """W = 260 with |shiftx| <= 3: an edge tile, an interior tile and a partial edge tile of
    k_stack_hist; the redo pixels of the marked columns go to k_stack_sorted<16, true> and
    k_stack_replay<2048> (513, 1024), to the replay and literal kernels (1025 .. 2047), to the
    literal kernel alone (from 2049)"""
    r = _hist_run(gpu_ctx, N, kind)
    assert r["path"] == 1
    assert_same(r["out"], r["ref"], f"hist N={N} {kind}")
    assert np.array_equal(r["rej"], r["rej_ref"]), (r["rej"], r["rej_ref"])


@gpu
@pytest.mark.parametrize("N,kind", [c for c in HIST_CASES if c[1] in ("sigma", "winsorized")])
def test_fast_path_carries_the_noise_columns(gpu_ctx, N, kind):
    """the histogram kernel decides the plain columns itself: its redo list holds at most the pixels
    a marked column or an emptied row touches plus 10 % of the rest (rounding-band and early-break
    pixels).  A build that sent everything to the redo list would still pass the parity test"""
    r = _hist_run(gpu_ctx, N, kind)
    touched = int(r["touched"].sum())
    rest = r["touched"].size - touched
    print(f"N={N} {kind}: chain_pixels={r['chain_pixels']} touched={touched} rest={rest}")
    assert rest >= 500, rest
    assert r["chain_pixels"] <= touched + 0.10 * rest, (r["chain_pixels"], touched, rest)


@gpu
@pytest.mark.parametrize("kind", ["sigma", "winsorized"])
@pytest.mark.parametrize("N", [1024, 1025, 1449])
@pytest.mark.parametrize("normalize", [sg.ADDITIVE_SCALING, sg.MULTIPLICATIVE_SCALING])
def test_hist_route_normalised_across_counts(gpu_ctx, normalize, N, kind):
    """normalised loads: the compact side list exists up to 1024 frames (the sorted kernel reads
    it) and not beyond; 1449 runs the normalised integer-moment WINSORIZED branch"""
    H, mt, ms = _geom(N)
    sx, sy = orc.synth_shifts(N, seed=N, maxshift=ms)
    frames = _captured_trio(_columns(N, H, 260, N)[0], sx, sy)
    ref, rej_ref, out, rej, st = _stack_both(gpu_ctx, frames, kind, sx, sy, mt, normalize,
                                             _coeffs(normalize, N, seed=N + normalize))
    assert st.path == 1
    print(f"N={N} {kind} norm={normalize}: compact_pixels={st.compact_pixels} chain_pixels={st.chain_pixels}")
    if N <= 1024:
        assert st.compact_pixels > 0
    else:
        assert st.compact_pixels == 0
    assert_same(out, ref, f"hist N={N} {kind} norm={normalize}")
    assert np.array_equal(rej, rej_ref), (rej, rej_ref)


@gpu
@pytest.mark.parametrize("kind", ["sigma", "winsorized", "percentile", "sigmedian", "linearfit", "median"])
@pytest.mark.parametrize("N", [513, 1024])
def test_sorted_kernel_sixteen_registers(gpu_ctx, N, kind):
    """k_stack_sorted<16, false> over every tile (kernel_path = PATH_SORTED): 16 samples per lane,
    the largest LDS stage (132 N bytes); W = 130: the third 64-pixel tile holds 2 pixels"""
    H, mt, ms = _geom(N)
    frames, _ = _columns(N, H, 130, 7 * N)
    sx, sy = orc.synth_shifts(N, seed=7 * N, maxshift=ms)
    ref, rej_ref, out, rej, st = _stack_both(gpu_ctx, frames, kind, sx, sy, mt, kernel_path=sg.PATH_SORTED)
    assert st.path == 0
    assert_same(out, ref, f"sorted N={N} {kind}")
    assert np.array_equal(rej, rej_ref), (rej, rej_ref)


def _device_stack(ctx, dev_frames, desc, C, H, W):
    """a stack of frames already on the device (torch int16 tensor): (image, counters, maximum)"""
    import torch
    o = torch.zeros(C * H * W, dtype=torch.int16, device="cuda")
    torch.cuda.synchronize()            # the library runs on its own (non-blocking) stream
    rej, maxim = ctx.stack_device(desc, dev_frames.data_ptr(), C * H * W, H * W, o.data_ptr(), 0, H)
    return o.cpu().numpy().view(np.uint16).reshape(C, H, W), rej, maxim


def _upload(frames):
    import torch
    with warnings.catch_warnings():     # the cached frames are read only; they are only copied from
        warnings.simplefilter("ignore", UserWarning)
        return torch.from_numpy(np.ascontiguousarray(frames).view(np.int16).reshape(-1)).cuda()


BOUNDARY_W, BOUNDARY_H = 130, 4
BOUNDARY_SAT, BOUNDARY_HALF = (1, 40), (2, 100)         # (row, x) of the two marked columns


@functools.lru_cache(maxsize=1)
def _boundary_frames(N, mix="zeros"):
    """background as `_columns` with a random 60 % of every column's frames at 0 (about 26 k in-band
    samples, at most ~210 per bin; the zeros go through the 16-bit zero counters), one all-65535
    column and one half dark / half bright column.  Such a column's median is 0, outside the band,
    so the histogram kernel counts it and hands it to the redo list.  mix = "split": 43 % of the
    frames at 0, 44 % at 65535 and 13 % in the band (about 8.5 k samples, at most ~220 per bin), so
    the median rank lies in the band (as the first 16 frames, which place the band) and the histogram
    kernel decides the column itself, with the largest moments it can meet (n SS - S^2 near
    n^2 65535^2 / 4 = 2^62)"""
    H, W = BOUNDARY_H, BOUNDARY_W
    rng = np.random.default_rng(N)
    f = np.rint(1000.0 + 20.0 * rng.standard_normal(size=(N, 1, H, W), dtype=np.float32)).astype(np.uint16)
    u = rng.random(f.shape, dtype=np.float32)
    if mix == "split":
        u[:16] = 0.5        # the band centre is the median of the first 16 frames: keep them in the band
        f[u < 0.43] = 0
        f[u >= 0.56] = 65535
    else:
        f[u < 0.6] = 0
    del u
    f[:, 0, BOUNDARY_SAT[0], BOUNDARY_SAT[1]] = 65535
    f[:, 0, BOUNDARY_HALF[0], BOUNDARY_HALF[1]] = np.rint(rng.normal(60000.0, 20.0, size=N))
    f[rng.permutation(N)[: N // 2], 0, BOUNDARY_HALF[0], BOUNDARY_HALF[1]] = 0
    f.setflags(write=False)
    return f


@gpu
@pytest.mark.parametrize("N,kind,path,mix", [(65535, "sigma", 1, "zeros"), (65535, "winsorized", 1, "zeros"),
                                             (65536, "sigma", 0, "zeros"), (65535, "sigma", 1, "split")])
def test_hist_to_literal_boundary(gpu_ctx, N, kind, path, mix):
    """the last frame count of the histogram path and the first one beyond it (every pixel to the
    literal kernel, one thread sorting 65536 samples out of scratch).  With 60 % zeros ("zeros") a
    column's median is 0, outside the band: at 65535 frames the histogram kernel builds and counts
    every column (39 k zeros in the 16-bit halves) and hands 519 of the 520 pixels to the literal
    kernel; "split" keeps the median in the band, and the histogram kernel decides all but the
    half dark / half bright pixel itself, with moments near 2^62.

    Measured on an MI355X, the GPU call (sg_stack_stats.total_ms) and the whole test:
      65535 SIGMA zeros        0.89 s    2.3 s
      65535 WINSORIZED zeros  89.6 s   107 s  (93.2 s / 111 s in a second run; the oracle takes 32 s of it)
      65536 SIGMA zeros        0.89 s    2.3 s
      65535 SIGMA split        0.44 s    2.3 s
    The WINSORIZED case is far over 20 s and wider sigmas do not shorten it: the median is 0, so each
    Winsorize iteration shrinks sigma by a constant factor (0.83) until it underflows, thousands of
    inner iterations over 65535 samples whatever the sigmas are (the oracle takes 31 - 33 s and
    returns the same counters at (3, 3), (5, 5) and (8, 8)); the clipping pass then rejects every
    non-zero sample.  The case is kept as it is."""
    C, H, W = 1, BOUNDARY_H, BOUNDARY_W
    frames = _boundary_frames(N, mix)
    rc, ref, rej_ref = orc.stack_rejection(frames, REJ[kind], sig=SIG[kind], max_thread=1)
    assert rc == 0
    desc, keep = sg.make_desc(sg.MEAN, N, W, H, C, rejection=REJ[kind], sig=SIG[kind], max_thread=1,
                              max_number_of_rows=H)
    dev = _upload(frames)
    out, rej, _ = _device_stack(gpu_ctx, dev, desc, C, H, W)
    st = gpu_ctx.stats()
    print(f"N={N} {kind} {mix}: path={st.path} chain_pixels={st.chain_pixels} slow_pixels={st.slow_pixels} "
          f"total_ms={st.total_ms:.1f}")
    assert st.path == path
    assert_same(out, ref, f"boundary N={N} {kind} {mix}")
    assert np.array_equal(rej, rej_ref), (rej, rej_ref)
    if mix == "split":  # the background columns are decided in the histogram kernel
        assert st.chain_pixels <= 2 + 0.10 * H * W, st.chain_pixels


SUM_FRAMES = 65538
SUM_ODD_FRAME = 5                                       # the frame where the "all but one" pixels hold noise
SUM_SHAPES = {"small": (8, [(0, 1)], [(0, 2)]),
              "wide": (600, [(0, 1)] + [(0, x) for x in range(300, 305)], [(0, 2)] + [(0, x) for x in range(310, 315)])}


@functools.lru_cache(maxsize=2)
def _sum_frames(shape, H):
    """SUM_FRAMES frames of noise around 30000 (uniform in 29000..31000); `full` pixels at 65535 in
    every frame (N 65535 is 2^32 - 1 at 65537 frames and wraps a uint32_t at 65538), `but one`
    pixels at 65535 in every frame but SUM_ODD_FRAME.  The wide shape repeats both over 5 adjacent
    pixels, so that under |shiftx| <= 2 the middle output pixel still collects 65535 from every
    frame"""
    W, full, butone = SUM_SHAPES[shape]
    rng = np.random.default_rng(H * 1000 + W)
    f = rng.integers(29000, 31001, size=(SUM_FRAMES, 1, H, W), dtype=np.uint16)
    for (r, x) in full:
        f[:, 0, r, x] = 65535
    for (r, x) in butone:
        keep = f[SUM_ODD_FRAME, 0, r, x]
        f[:, 0, r, x] = 65535
        f[SUM_ODD_FRAME, 0, r, x] = keep
    f.setflags(write=False)
    return f


def _sum_shifts(shape, N):
    """none at the small shape; |shiftx| <= 2 at the wide one (k_stack_reduce3's interior segments
    at 128, 256 and 384 and its edge segments), no row shifts: a row shift would empty the rows"""
    if shape == "small":
        return None, None
    sx, _ = orc.synth_shifts(N, seed=N, maxshift=2)
    return sx, np.zeros(N, np.int32)


@gpu
@pytest.mark.parametrize("N", [65537, 65538])
@pytest.mark.parametrize("kind", ["sum", "mean", "mean-additive"])
@pytest.mark.parametrize("shape", ["small", "wide"])
def test_reduce_sum_width(gpu_ctx, shape, kind, N):
    """SUM and MEAN without rejection at N 65535 = 2^32 - 1 (the uint32_t kernels' last count) and
    one frame more (64-bit sums and maximum): SUM's image and maximum == stack_summing's unsigned
    long sums, MEAN's image == the reference's sum / N in double.  SUM at H = 2 and 1; MEAN at
    H = 4 (the reference's block partition needs four rows)"""
    C, W = 1, SUM_SHAPES[shape][0]
    H = 4 if kind != "sum" else 2 if shape == "small" else 1
    frames = _sum_frames(shape, H)[:N]
    sx, sy = _sum_shifts(shape, N)
    full = SUM_SHAPES[shape][1][-3 if shape == "wide" else 0]       # collects 65535 from every frame
    dev = _upload(frames)
    if kind == "sum":
        rc, ref, mref = orc.stack_sum(frames, sx, sy)
        assert rc == 0 and mref == N * 65535, mref
        desc, keep = sg.make_desc(sg.SUM, N, W, H, C, shiftx=sx, shifty=sy)
        out, _, maxim = _device_stack(gpu_ctx, dev, desc, C, H, W)
        assert maxim == mref, (maxim, mref)
    else:
        normalize, off, sc = sg.NO_NORM, None, None
        if kind == "mean-additive":     # scales >= 1, offsets <= 0: a 65535 sample stays 65535, the sum still wraps
            rng = np.random.default_rng(N)
            normalize, off, sc = sg.ADDITIVE_SCALING, -40.0 * rng.random(N), 1.0 + 0.01 * rng.random(N)
        rc, ref, _ = orc.stack_rejection(frames, sg.NO_REJEC, shiftx=sx, shifty=sy, normalize=normalize, offset=off,
                                         scale=sc, max_thread=1)
        assert rc == 0 and ref[0, full[0], full[1]] == 65535
        desc, keep = sg.make_desc(sg.MEAN, N, W, H, C, rejection=sg.NO_REJEC, normalize=normalize, shiftx=sx, shifty=sy,
                                  offset=off, scale=sc, max_thread=1, max_number_of_rows=H)
        out, _, _ = _device_stack(gpu_ctx, dev, desc, C, H, W)
    assert gpu_ctx.stats().path == 0
    assert_same(out, ref, f"{kind} {shape} N={N}")


# ---- CPU-only premise tests: what the GPU tests above take for granted about their inputs ----

def _moment_terms(col):
    v = [int(x) for x in col]
    n, S, SS = len(v), sum(v), sum(x * x for x in v)
    return n * SS, S * S


def test_wide_moments_premise():
    """n SS - S^2 of the half dark / half bright column (exact Python integers; the difference does
    not depend on the origin the kernel counts from): past 2^53 at 4099 frames, so a double cannot
    hold it exactly and sgh_sigma_fast's conversion rounds; at 65535 frames n SS is past 2^62 and
    the difference past 2^61.  (65535 32768 60000^2 = 7.7e18 stays below 2^63 = 9.2e18, and
    n SS - S^2 <= n^2 65535^2 / 4 < 2^62 for any column of at most 65535 samples: the kernels'
    signed 64-bit moments hold every value they can meet.)"""
    f, _ = _columns(4099, 8, 260, 4099)
    x = _run_starts(260)[3]
    nss, s2 = _moment_terms(f[:, 0, 4, x])
    assert nss - s2 >= 2 ** 53
    b = _boundary_frames(65535)
    nss, s2 = _moment_terms(b[:, 0, BOUNDARY_HALF[0], BOUNDARY_HALF[1]])
    assert 2 ** 62 <= nss < 2 ** 63 and s2 >= 2 ** 61 and nss - s2 >= 2 ** 61
    assert 65535 ** 2 * 65535 ** 2 // 4 < 2 ** 62


@pytest.mark.parametrize("N", HIST_COUNTS)
def test_fast_path_columns_premise(N):
    """every unmarked column of `_columns` fits the histogram kernel's fast path: no value more
    than 255 times (the u8 bins) and no sample further than 100 from the median of the first 16
    frames (the band is 256 bins around it); enough of them remain for the carry condition"""
    H, _, ms = _geom(N)
    f, marked = _columns(N, H, 260, N)
    cols = f[:, 0][:, ~marked].astype(np.int32)                 # [N][unmarked]
    centre = np.median(cols[:16], axis=0)
    assert (np.abs(cols - centre) <= 100).all()
    off = cols - cols.min()
    counts = np.bincount((off * cols.shape[1] + np.arange(cols.shape[1])[None, :]).ravel())
    assert counts.max() <= 255, counts.max()
    assert marked.sum() <= 9 * RUN_LEN + 40, marked.sum()
    sx, sy = orc.synth_shifts(N, seed=N, maxshift=ms)
    assert (~_touched(marked, sx, sy)).sum() >= 500


def test_u32_limits_premise():
    assert 65537 * 65535 == 2 ** 32 - 1 and 65538 * 65535 > 2 ** 32 - 1
    f = _sum_frames("small", 2)
    assert (f[:, 0, 0, 1] == 65535).all() and (f[:, 0, 0, 2] == 65535).sum() == SUM_FRAMES - 1
    assert int(f[:65537, 0].astype(np.uint64).sum(axis=0).max()) == 2 ** 32 - 1
