"""Star candidates on the device (sg_findstar*) against tests/findstar_ref.py, bit
for bit: the detection plane over the tile grid's cases, the threshold records, the peak test with
its tie rule, the ordered and capped candidate list, the boxes, frame strides and layers, the host
entry and the refused arguments.  tests/test_findstar_cpu.py holds, for the same images, that a
wrong filter order, tie rule, list order or summation order would change what is compared here."""
import numpy as np
import pytest

import findstar_ref as fr
import sirilgpu as sg

pytestmark = pytest.mark.gpu

GAP_FILL = 0xABCD
XY_FILL = -77


def _run(ctx, frames, r, k, layer=0, area=None, maxc=64, gap=0, want_boxes=True, want_wave=True):
    """sg_findstar_device on frames [N][C][H][W], C*H*W + gap samples apart.  The frames, the gaps and
    the guards after the last frame and after the planes must come back untouched.
    Returns (rc, records, xy, boxes, wave[N][H][W] or None)."""
    import torch
    N, C, H, W = frames.shape
    total = C * H * W
    stride = total + gap
    buf = np.full(N * stride + 64, GAP_FILL, dtype=np.uint16)
    for i in range(N):
        buf[i * stride:i * stride + total] = frames[i].reshape(-1)
    d = torch.from_numpy(buf.view(np.int16).copy()).cuda()
    wbuf = np.full(N * H * W + 64, GAP_FILL, dtype=np.uint16)
    dw = torch.from_numpy(wbuf.view(np.int16).copy()).cuda() if want_wave else None
    torch.cuda.synchronize()
    rc, rec, xy, bx = ctx.findstar_device(d.data_ptr(), N, C, H, W, r, k, layer=layer, area=area, max_candidates=maxc,
                                          want_boxes=want_boxes, d_wave=dw.data_ptr() if want_wave else None,
                                          frame_stride=stride if gap else 0)
    torch.cuda.synchronize()
    assert np.array_equal(d.cpu().numpy().view(np.uint16), buf), "the frames, a gap or the guard changed"
    wave = None
    if want_wave:
        got = dw.cpu().numpy().view(np.uint16)
        assert (got[N * H * W:] == GAP_FILL).all(), "guard after the planes written"
        wave = got[:N * H * W].reshape(N, H, W)
    return rc, rec, xy, bx, wave


def _same(a, b):
    return np.float64(a).tobytes() == np.float64(b).tobytes()


def _check_record(q, want, ncand=None, maxc=None):
    assert q.ngood == want["ngood"] and q.no_data == want["no_data"]
    assert _same(q.median, want["median"]) and _same(q.sigma, want["sigma"]), (q.median, q.sigma, want)
    assert q.threshold == want["threshold"] and q.threshold_wrapped == want["wrapped"], (q.threshold, want)
    if ncand is not None:
        assert q.ncand == ncand and q.nstored == min(ncand, maxc), (q.ncand, q.nstored, ncand)


def _check(ctx, frames, r, k, layer=0, area=None, maxc=64, gap=0, want_boxes=True):
    """the whole answer of every frame against the reference; returns the candidate lists"""
    rc, rec, xy, bx, wave = _run(ctx, frames, r, k, layer, area, maxc, gap, want_boxes)
    assert rc == 0, ctx.error()
    lists = []
    for f in range(frames.shape[0]):
        plane = frames[f, layer]
        cands, want, wref = fr.candidates(plane, k, r, area)
        assert np.array_equal(wave[f], wref), (f, np.argwhere(wave[f] != wref)[:5])
        _check_record(rec[f], want, len(cands), maxc)
        assert rec[f].wavelet_applied == int(min(plane.shape) >= 32) and rec[f].ratio_applied == 0
        assert rec[f].sigma_on_host == 0
        n = min(len(cands), maxc)
        assert xy[f, :n].tolist() == [list(c) for c in cands[:n]], (f, xy[f, :n].tolist(), cands[:n])
        assert (xy[f, n:] == 0).all()
        if want_boxes:
            assert np.array_equal(bx[f, :n], fr.boxes(plane, cands[:n], r))
            assert (bx[f, n:] == 0).all()
        lists.append(cands)
    return lists


# ------------------------------------------------------------------ detection plane

@pytest.mark.parametrize("H,W", fr.PLANE_SHAPES)
def test_detection_plane(gpu_ctx, H, W):
    img = fr.plane_case(H, W)
    rc, rec, _, _, wave = _run(gpu_ctx, img[None, None], 3, 1.0)
    assert rc == 0, gpu_ctx.error()
    want, applied, ratio = fr.detection_plane(img)
    assert applied == 1 and rec[0].wavelet_applied == 1 and rec[0].ratio_applied == ratio == 0
    assert np.array_equal(wave[0], want), np.argwhere(wave[0] != want)[:5]
    assert (want != fr.detection_plane(img, fr.smooth_separable)[0]).any()


@pytest.mark.parametrize("H,W", [(31, 64), (64, 31)])
def test_no_wavelet_plane_is_the_image(gpu_ctx, H, W):
    img = fr.noise_frame(7 + W, H, W)
    rc, rec, _, _, wave = _run(gpu_ctx, img[None, None], 3, 1.0)
    assert rc == 0 and rec[0].wavelet_applied == 0 and rec[0].ratio_applied == 0
    assert np.array_equal(wave[0], img)
    _check(gpu_ctx, img[None, None], 3, 0.5, maxc=512)


# ------------------------------------------------------------------ threshold records

def _record_frames():
    rng = np.random.default_rng(11)
    H, W = 40, 48
    zeros = rng.integers(0, 3000, size=(H, W)).astype(np.uint16)
    zeros[rng.random((H, W)) < 0.3] = 0
    sat = rng.integers(1, 60000, size=(H, W)).astype(np.uint16)
    sat[rng.random((H, W)) < 0.2] = 65535
    half = rng.integers(100, 900, size=(H, W)).astype(np.uint16)
    half[rng.random((H, W)) < 0.6] = 65535
    single = np.zeros((H, W), dtype=np.uint16)
    single[17, 29] = 4242
    return dict(zeros=zeros, sat=sat, half=half, single=single)


@pytest.mark.parametrize("name", ["zeros", "sat", "half", "single"])
def test_threshold_records(gpu_ctx, name):
    img = _record_frames()[name]
    want = fr.threshold(img, 1.0)
    if name == "half":
        assert want["median"] == 0.0 and (img == 65535).sum() * 2 > img.size
    if name == "single":
        assert want["ngood"] == 1 and want["sigma"] == 0.0
    _check(gpu_ctx, img[None, None], 3, 1.0, maxc=256)


def test_all_zero_frame_in_the_middle(gpu_ctx):
    a, _ = fr.star_case(0)
    frames = np.stack([a, np.zeros_like(a), a[::-1].copy()])[:, None]
    lists = _check(gpu_ctx, frames, 5, 1.0)
    assert lists[1] == [] and len(lists[0]) >= 2 and len(lists[2]) >= 2
    rc, rec, *_ = _run(gpu_ctx, frames, 5, 1.0)
    assert rc == 0 and [q.no_data for q in rec] == [0, 1, 0] and rec[1].ncand == 0 and rec[1].ngood == 0


def test_threshold_wraps(gpu_ctx):
    img, r = fr.star_case(0)
    lists = _check(gpu_ctx, img[None, None], r, 100.0, maxc=512)
    rc, rec, *_ = _run(gpu_ctx, img[None, None], r, 100.0)
    assert rc == 0 and rec[0].threshold_wrapped == 1 and rec[0].threshold == fr.threshold(img, 100.0)["threshold"]
    assert lists[0] == fr.peaks(fr.detection_plane(img)[0], rec[0].threshold, r)


def test_sigma_on_host_above_2_53(gpu_ctx):
    img = fr.bright_frame()
    want = fr.threshold(img, 1.0)
    exact, s2 = fr.sigma_from_sums(img)
    assert s2 >= 2 ** 53 and not _same(exact, want["sigma"])
    rc, rec, *_ = _run(gpu_ctx, img[None, None], 10, 1.0, maxc=0, want_boxes=False, want_wave=False)
    assert rc == 0, gpu_ctx.error()
    assert rec[0].sigma_on_host == 1
    _check_record(rec[0], want)


# ------------------------------------------------------------------ peak test

def test_tie_rule(gpu_ctx):
    img = fr.tie_image()
    lists = _check(gpu_ctx, img[None, None], 1, 1.0, maxc=4096)
    thr = fr.threshold(img, 1.0)["threshold"]
    assert lists[0] != fr.peaks(img, thr, 1, rule="gt_only") and lists[0] != fr.peaks(img, thr, 1, rule="ge_all")


def test_noise_frame(gpu_ctx):
    lists = _check(gpu_ctx, fr.noise_frame(64, 64, 64)[None, None], 2, 0.0, maxc=4096)
    assert len(lists[0]) > 10


@pytest.mark.parametrize("case", [0, 1])
def test_star_fields(gpu_ctx, case):
    img, r = fr.star_case(case)
    lists = _check(gpu_ctx, img[None, None], r, 1.0)
    assert len(lists[0]) >= 2


def test_radius_one(gpu_ctx):
    img, _ = fr.star_case(1)
    lists = _check(gpu_ctx, img[None, None], 1, 1.0, maxc=512)
    assert len(lists[0]) >= 2


def test_radius_covers_the_image(gpu_ctx):
    img, _ = fr.star_case(0)                    # 40 x 48
    for r in (20, 24, 1000):
        rc, rec, xy, bx, wave = _run(gpu_ctx, img[None, None], r, 1.0, maxc=4)
        assert rc == 0 and rec[0].ncand == 0 and rec[0].nstored == 0 and (xy == 0).all() and (bx == 0).all()
        assert np.array_equal(wave[0], fr.detection_plane(img)[0])
        _check_record(rec[0], fr.threshold(img, 1.0))


def test_area_with_odd_offsets(gpu_ctx):
    img, _ = fr.star_case(1)                    # 96 x 130
    area = (7, 11, 101, 63)
    lists = _check(gpu_ctx, img[None, None], 3, 1.0, area=area, maxc=512)
    whole = fr.candidates(img, 1.0, 3)[0]
    assert 2 <= len(lists[0]) < len(whole)
    assert lists[0] == [c for c in whole if 10 <= c[0] < 105 and 14 <= c[1] < 71]
    _check(gpu_ctx, img[None, None], 3, 1.0, area=(7, 11, 6, 63))          # 2r >= the area's width: empty


# ------------------------------------------------------------------ capacity, boxes

@pytest.mark.parametrize("maxc", [10, 0])
def test_capacity(gpu_ctx, maxc):
    img = fr.noise_frame(64, 64, 64)
    full = fr.candidates(img, 0.0, 2)[0]
    assert len(full) > 10
    rc, rec, xy, bx, _ = _run(gpu_ctx, img[None, None], 2, 0.0, maxc=maxc)
    assert rc == 0 and rec[0].ncand == len(full) and rec[0].nstored == maxc
    assert xy.shape == (1, maxc, 2) and xy[0].tolist() == [list(c) for c in full[:maxc]]
    assert np.array_equal(bx[0], fr.boxes(img, full[:maxc], 2))


@pytest.mark.parametrize("case,r", [(1, 1), (1, 10)])
def test_boxes_entry_by_entry(gpu_ctx, case, r):
    img, _ = fr.star_case(case)
    rc, rec, xy, bx, _ = _run(gpu_ctx, img[None, None], r, 1.0, maxc=64)
    assert rc == 0 and rec[0].nstored >= 2
    top = img[::-1]
    for n in range(rec[0].nstored):
        x, y = xy[0, n]
        for ii in range(2 * r):
            for jj in range(2 * r):
                assert bx[0, n, ii, jj] == top[y - r + jj, x - r + ii], (n, ii, jj)
    rc2, rec2, xy2, none, _ = _run(gpu_ctx, img[None, None], r, 1.0, maxc=64, want_boxes=False)
    assert rc2 == 0 and none is None and np.array_equal(xy2, xy) and rec2[0].ncand == rec[0].ncand


# ------------------------------------------------------------------ plumbing

def _three_frames():
    imgs = [fr.star_field(300 + i, 40, 48, 5, margin=8) for i in range(9)]
    return np.stack(imgs).reshape(3, 3, 40, 48)


def test_layers_and_frame_stride(gpu_ctx):
    frames = _three_frames()
    lists = _check(gpu_ctx, frames, 4, 1.0, layer=1, gap=7)
    assert all(len(c) >= 1 for c in lists) and lists[0] != lists[1]
    for layer in (0, 2):
        _check(gpu_ctx, frames, 4, 1.0, layer=layer, gap=7)


def test_host_entry(gpu_ctx):
    frames = _three_frames()
    rc, rec, xy, bx, wave = gpu_ctx.findstar(frames, 4, 1.0, layer=1, max_candidates=32, want_wave=True)
    assert rc == 0, gpu_ctx.error()
    rcd, recd, xyd, bxd, waved = _run(gpu_ctx, frames, 4, 1.0, layer=1, maxc=32)
    assert rcd == 0 and np.array_equal(xy, xyd) and np.array_equal(bx, bxd) and np.array_equal(wave, waved)
    for a, b in zip(rec, recd):
        assert bytes(a) == bytes(b)
    assert sum(q.nstored for q in rec) >= 3
    rc, rec2, xy2, none, nowave = gpu_ctx.findstar(frames, 4, 1.0, layer=1, max_candidates=32, want_boxes=False)
    assert rc == 0 and none is None and nowave is None and np.array_equal(xy2, xy)


BAD = [
    (dict(W=0), sg.SG_ERR_SIZE), (dict(H=-1), sg.SG_ERR_SIZE), (dict(C=0), sg.SG_ERR_SIZE),
    (dict(W=65536, H=32768), sg.SG_ERR_SIZE), (dict(layer=3), sg.SG_ERR_SIZE), (dict(layer=-1), sg.SG_ERR_SIZE),
    (dict(area=(-1, 0, 10, 10)), sg.SG_ERR_SIZE), (dict(area=(40, 0, 10, 10)), sg.SG_ERR_SIZE),
    (dict(area=(0, 35, 10, 10)), sg.SG_ERR_SIZE), (dict(radius=0), sg.SG_ERR_GENERIC),
    (dict(radius=-2), sg.SG_ERR_GENERIC), (dict(sigma=-1.0), sg.SG_ERR_GENERIC),
    (dict(sigma=float("nan")), sg.SG_ERR_GENERIC), (dict(sigma=float("inf")), sg.SG_ERR_GENERIC),
    (dict(maxc=-1), sg.SG_ERR_GENERIC),
]


def test_refused_arguments_touch_nothing(gpu_ctx):
    import ctypes
    import torch
    frames = _three_frames()
    d = torch.from_numpy(frames.view(np.int16).reshape(-1).copy()).cuda()
    dw = torch.full((3 * 40 * 48,), 0x1234, dtype=torch.int16, device="cuda")
    torch.cuda.synchronize()
    for change, code in BAD:
        a = dict(W=48, H=40, C=3, layer=1, radius=4, sigma=1.0, area=None, maxc=8)
        a.update(change)
        desc = sg.make_findstar_desc(a["W"], a["H"], a["C"], a["layer"], a["radius"], a["sigma"], a["area"], a["maxc"])
        rec = (sg.FindstarFrame * 3)()
        xy = np.full((3, 8, 2), XY_FILL, dtype=np.int32)
        bx = np.full((3, 8, 8, 8), GAP_FILL, dtype=np.uint16)
        rc = gpu_ctx.lib.sg_findstar_device(gpu_ctx.ctx, 0, ctypes.byref(desc), ctypes.c_void_p(d.data_ptr()), 3, 0, rec,
                                            xy.ctypes.data_as(ctypes.c_void_p), bx.ctypes.data_as(ctypes.c_void_p),
                                            ctypes.c_void_p(dw.data_ptr()), None)
        assert rc == code, (change, rc, gpu_ctx.error())
        assert gpu_ctx.error(), change
        assert (xy == XY_FILL).all() and (bx == GAP_FILL).all()
        rch = gpu_ctx.lib.sg_findstar(gpu_ctx.ctx, ctypes.byref(desc), frames.ctypes.data_as(ctypes.c_void_p), 3, rec,
                                      xy.ctypes.data_as(ctypes.c_void_p), bx.ctypes.data_as(ctypes.c_void_p), None)
        assert rch == code and (xy == XY_FILL).all()
    torch.cuda.synchronize()
    assert np.array_equal(d.cpu().numpy().view(np.uint16), frames.reshape(-1))
    assert (dw.cpu().numpy() == 0x1234).all()
