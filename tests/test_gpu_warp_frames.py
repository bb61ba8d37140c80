"""sg_warp_frames_u16* (the sequence warp) on the GPU: every written byte equals tests/warp_ref.py and the
single-frame entry sg_warp_u16_device on the same frame, whatever route a tile takes (LDS or global
memory: the default route of each interpolation, SG_WARP_ROUTE=1 and SG_WARP_ROUTE=2); actions, slots and
pitches leave everything else at the sentinel; the counters prove the routes; the caller's stream, the
host entry and its batch loop; the refusals."""
import functools
import os

import numpy as np
import pytest

import sirilgpu as sg
import warp_cases as wc
import warp_ref
from test_warp import _feat, _rot

pytestmark = pytest.mark.gpu

N, W, H = 5, wc.W, wc.H
SENT = 0xA5C3
MIXED = ("shift_frac", "rot5", "rot45", "scale1_25", "perspective")      # five different homographies
HARD = ("horizon", "singular", "rot90", "scale0_8", "rot0_5")
OUT_SIZES = [(96, 80), (150, 40), (150, 9), (70, 50)]
SKIP, APPLY, COPY = sg.WARP_SKIP, sg.WARP_APPLY, sg.WARP_COPY
ACTIONS, SLOTS = [APPLY, SKIP, COPY, APPLY, SKIP], [0, -1, 1, 2, -1]
TILE_X, TILE_Y = 64, 16
LDS_DEFAULT = (1, 2, 4)       # the interpolations whose default route is LDS (sg_warp_plan.hpp)


@functools.lru_cache(maxsize=None)
def _frames(C):
    f = wc.frames(N, 3)[:, :C].copy()
    f.setflags(write=False)
    return f


@functools.lru_cache(maxsize=None)
def _want(C, names, out_size, interp):
    """warp_ref per frame, [N][C][oH][oW]; computed once per case and shared"""
    w = np.stack([warp_ref.warp(_frames(C)[f], wc.HOMS[names[f]], out_size, interp) for f in range(N)])
    w.setflags(write=False)
    return w


def _homs(names):
    return np.stack([wc.HOMS[n] for n in names])


def _context(**env):
    """a context created under the given knobs (they are read once, at sg_init)"""
    old = {k: os.environ.get(k) for k in env}
    os.environ.update({k: str(v) for k, v in env.items()})
    try:
        return sg.Context([0])
    finally:
        for k, v in old.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v


@pytest.fixture(scope="module")
def ctx_gather(gpu_ctx):
    c = _context(SG_WARP_ROUTE=1)
    yield c
    c.close()


@pytest.fixture(scope="module")
def ctx_lds(gpu_ctx):
    """nearest and cubic gather by default (the measured faster way): their LDS route runs under SG_WARP_ROUTE=2"""
    c = _context(SG_WARP_ROUTE=2)
    yield c
    c.close()


@pytest.fixture(scope="module")
def ctx_batch2(gpu_ctx):
    c = _context(SG_HOST_BATCH=2)
    yield c
    c.close()


def _to_dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint16).view(np.int16).copy()).cuda()


def _device(ctx, frames, homs, out_size, interp, action=None, out_slot=None, nslots=None, fgap=0, ogap=0):
    """sg_warp_frames_u16_device on frames [n][C][h][w]; returns (rc, out [nslots][frame + ogap] u16) of an output
    buffer pre-filled with SENT; the source, laid out with fgap elements between frames, must come back unchanged"""
    import torch
    n, C, h, w = frames.shape
    oW, oH = out_size if out_size else (w, h)
    ie, oe = C * h * w, C * oH * oW
    nslots = n if nslots is None else nslots
    src = np.full((n, ie + fgap), 0x1234, dtype=np.uint16)
    src[:, :ie] = frames.reshape(n, ie)
    d_in = _to_dev(src)
    d_out = _to_dev(np.full((nslots, oe + ogap), SENT, dtype=np.uint16))
    rc = ctx.warp_frames_device(d_in.data_ptr(), n, w, h, C, d_out.data_ptr(), oW, oH, homs, interp, action=action,
                                out_slot=out_slot, frame_pitch=ie + fgap if fgap else 0, out_frame_pitch=oe + ogap if ogap else 0)
    torch.cuda.synchronize()
    assert np.array_equal(d_in.cpu().numpy().view(np.uint16), src)
    return rc, d_out.cpu().numpy().view(np.uint16)


def _single(ctx, frames, homs, out_size, interp):
    """sg_warp_u16_device frame by frame"""
    import torch
    n, C, h, w = frames.shape
    oW, oH = out_size if out_size else (w, h)
    d_in = _to_dev(frames)
    d_out = torch.zeros(n * C * oH * oW, dtype=torch.int16, device="cuda")
    for f in range(n):
        ctx.warp_device(d_in.data_ptr() + 2 * f * C * h * w, w, h, C, d_out.data_ptr() + 2 * f * C * oH * oW, oW, oH, homs[f], interp)
    torch.cuda.synchronize()
    return d_out.cpu().numpy().view(np.uint16).reshape(n, C, oH, oW)


def _tiles(out_size):
    return ((out_size[0] + TILE_X - 1) // TILE_X) * ((out_size[1] + TILE_Y - 1) // TILE_Y)


@pytest.mark.parametrize("out_size", OUT_SIZES)
@pytest.mark.parametrize("interp", [0, 1, 3, 4])
def test_equals_reference_and_single_frame_entry(gpu_ctx, ctx_gather, ctx_lds, interp, out_size):
    for C in (1, 3):
        for names in (MIXED, HARD):
            want = _want(C, names, out_size, interp)
            assert want.any()
            for ctx in (gpu_ctx, ctx_lds):
                rc, got = _device(ctx, _frames(C), _homs(names), out_size, interp)
                assert rc == 0, ctx.error()
                got = got.reshape(want.shape)
                assert np.array_equal(got, want), (C, names, ctx is ctx_lds, np.argwhere(got != want)[:5])
                ms, launches, lds, gather, stray = ctx.warp_frames_last_times()
                assert launches == 1 and lds + gather == _tiles(out_size) * N * C and stray == 0, (lds, gather, stray)
                assert ms > 0
                if ctx is ctx_lds or interp in LDS_DEFAULT:
                    assert lds > 0 and (gather == 0 or names is HARD), (names, lds, gather)
                else:
                    assert lds == 0
        one = _single(gpu_ctx, _frames(C), _homs(MIXED), out_size, interp)
        assert np.array_equal(one, _want(C, MIXED, out_size, interp))
        # every tile through global memory: the same bytes
        rc, got = _device(ctx_gather, _frames(C), _homs(MIXED), out_size, interp)
        assert rc == 0, ctx_gather.error()
        assert np.array_equal(got.reshape(one.shape), one)
        _, _, lds, gather, stray = ctx_gather.warp_frames_last_times()
        assert (lds, gather, stray) == (0, _tiles(out_size) * N * C, 0)


def test_area_is_linear(gpu_ctx):
    rc, got = _device(gpu_ctx, _frames(3), _homs(MIXED), (150, 40), 2)
    assert rc == 0, gpu_ctx.error()
    assert np.array_equal(got.reshape(N, 3, 40, 150), _want(3, MIXED, (150, 40), 1))
    assert np.array_equal(_want(3, MIXED, (150, 40), 1), np.stack([warp_ref.warp(_frames(3)[f], wc.HOMS[MIXED[f]], (150, 40), 2)
                                                                    for f in range(N)]))


@pytest.mark.parametrize("interp", [1, 4])
def test_actions_slots_and_pitches(gpu_ctx, interp):
    """COPY needs equal sizes, so the output is 96 x 80; 5 output frames, of which 0 .. 2 are written"""
    for C in (1, 3):
        want = _want(C, MIXED, (W, H), interp)
        for fgap, ogap in ((0, 0), (37, 53)):
            rc, got = _device(gpu_ctx, _frames(C), _homs(MIXED), (W, H), interp, action=ACTIONS, out_slot=SLOTS, fgap=fgap, ogap=ogap)
            assert rc == 0, gpu_ctx.error()
            e = C * H * W
            assert np.array_equal(got[0, :e], want[0].reshape(-1))
            assert np.array_equal(got[1, :e], _frames(C)[2].reshape(-1))          # the COPY frame equals its source
            assert np.array_equal(got[2, :e], want[3].reshape(-1))
            assert (got[3:] == SENT).all() and (got[:, e:] == SENT).all()
            _, _, lds, gather, stray = gpu_ctx.warp_frames_last_times()
            assert lds + gather == _tiles((W, H)) * 2 * C and stray == 0


def test_routes(gpu_ctx, ctx_lds):
    for ctx, interp in ((gpu_ctx, 4), (gpu_ctx, 1), (ctx_lds, 3), (ctx_lds, 0)):
        rc, got = _device(ctx, _frames(1), _homs(["rot5"] * N), (150, 40), interp)
        assert rc == 0, ctx.error()
        _, _, lds, gather, stray = ctx.warp_frames_last_times()
        assert (lds, gather, stray) == (9 * N, 0, 0), (interp, lds, gather, stray)
        assert np.array_equal(got.reshape(N, 1, 40, 150), _want(1, ("rot5",) * N, (150, 40), interp))
        rc, got = _device(ctx, _frames(1), _homs(["horizon"] * N), (150, 40), interp)
        assert rc == 0, ctx.error()
        _, _, lds, gather, stray = ctx.warp_frames_last_times()
        assert gather >= 3 * N and stray == 0 and lds + gather == 9 * N, (interp, lds, gather, stray)
        assert np.array_equal(got.reshape(N, 1, 40, 150), _want(1, ("horizon",) * N, (150, 40), interp))


@pytest.mark.parametrize("t", [1e7, -1e9])
def test_far_translation_is_zero(gpu_ctx, t):
    homs = np.stack([np.array([[1, 0, t], [0, 1, -t], [0, 0, 1.0]])] * 2)
    for interp in (0, 1, 3, 4):
        rc, got = _device(gpu_ctx, _frames(3)[:2], homs, (150, 40), interp)
        assert rc == 0 and not got.any(), interp


@pytest.mark.parametrize("interp", [3, 4])
def test_saturates_both_ends(gpu_ctx, interp):
    hom = np.array([[1, 0, 0.5], [0, 1, 0], [0, 0, 1.0]])
    frames = np.stack([_feat(3, seed=33), _feat(3, seed=34)])
    want = []
    for f in range(2):
        exp, sums = warp_ref.warp(frames[f], hom, None, interp, return_sums=True)
        assert sums.min() < -0.5 and sums.max() > 65535.5
        want.append(exp)
    rc, got = _device(gpu_ctx, frames, np.stack([hom] * 2), None, interp)
    assert rc == 0, gpu_ctx.error()
    assert np.array_equal(got.reshape(2, 3, 23, 31), np.stack(want))


def test_source_smaller_than_the_window(gpu_ctx):
    frames = np.stack([_feat(3, 2, 3, seed=50), _feat(3, 2, 3, seed=51)])       # 3 wide, 2 high
    homs = np.stack([np.eye(3), np.array(_rot(0.1, 0.3, -0.2))])
    for interp in (0, 1, 3, 4):
        for out_size in (None, (70, 20)):
            want = np.stack([warp_ref.warp(frames[f], homs[f], out_size, interp) for f in range(2)])
            rc, got = _device(gpu_ctx, frames, homs, out_size, interp)
            assert rc == 0, gpu_ctx.error()
            assert np.array_equal(got.reshape(want.shape), want), (interp, out_size)
    assert np.array_equal(warp_ref.warp(frames[0], homs[0], None, 4), frames[0])


def test_callers_stream(gpu_ctx):
    """queued on a stream of the caller's behind a late upload of the frames: see test_gpu_caller_stream.py"""
    import torch
    from test_gpu_caller_stream import _Late, _late_call
    C, out_size, interp = 3, (150, 40), 3
    want = _want(C, MIXED, out_size, interp)
    late = _Late(_frames(C))
    out = torch.zeros(want.size, dtype=torch.int16, device="cuda")
    keep = torch.zeros_like(out)
    rc = _late_call(late, lambda: gpu_ctx.warp_frames_device(late.ptr(), N, W, H, C, out.data_ptr(), out_size[0], out_size[1],
                                                              _homs(MIXED), interp, stream=late.stream), out=out)
    assert rc == 0, gpu_ctx.error()
    with torch.cuda.stream(late.s):
        keep.copy_(out, non_blocking=True)
    got = late.read(keep).reshape(want.shape)
    assert np.array_equal(got, want), np.argwhere(got != want)[:5]
    ms, launches, lds, gather, stray = gpu_ctx.warp_frames_last_times()
    assert launches == 1 and lds + gather == 9 * N * C and stray == 0


def test_host_entry_and_its_batches(gpu_ctx, ctx_batch2):
    for C in (1, 3):
        for interp, out_size in ((1, (150, 9)), (4, (70, 50))):
            want = _want(C, MIXED, out_size, interp)
            rc, got = gpu_ctx.warp_frames(_frames(C), _homs(MIXED), out_size, interp)
            assert rc == 0, gpu_ctx.error()
            assert np.array_equal(got, want)
            rc, got2 = ctx_batch2.warp_frames(_frames(C), _homs(MIXED), out_size, interp)        # batches 2 + 2 + 1
            assert rc == 0, ctx_batch2.error()
            assert np.array_equal(got2, want)
            _, launches, lds, gather, stray = ctx_batch2.warp_frames_last_times()
            assert launches == 3 and lds + gather == _tiles(out_size) * N * C and stray == 0
        # actions and slots across the batches; a permuted slot order as well
        want = _want(C, MIXED, (W, H), 3)
        for slots, order in ((SLOTS, (0, 2, 3)), ([2, -1, 0, 1, -1], (2, 3, 0))):
            outs = []
            for ctx in (gpu_ctx, ctx_batch2):
                out = np.full((N, C, H, W), SENT, dtype=np.uint16)
                rc, got = ctx.warp_frames(_frames(C), _homs(MIXED), (W, H), 3, action=ACTIONS, out_slot=slots, out=out)
                assert rc == 0 and got is out, ctx.error()
                outs.append(out)
            a, b, c = order        # the frames that land in slots 0, 1, 2
            for out in outs:
                for slot, f in enumerate((a, b, c)):
                    assert np.array_equal(out[slot], _frames(C)[f] if ACTIONS[f] == COPY else want[f]), (slots, slot)
                assert (out[3:] == SENT).all()
            assert np.array_equal(outs[0], outs[1])


def test_refusals_write_nothing(gpu_ctx):
    import torch
    C = 1
    e = C * H * W
    buf = _to_dev(np.full(2 * N * e, SENT, dtype=np.uint16))
    before = buf.cpu().numpy().copy()
    p = buf.data_ptr()
    homs = _homs(MIXED)

    def call(d_out=p + 2 * N * e, oW=W, oH=H, C=1, **kw):
        return gpu_ctx.warp_frames_device(p, N, W, H, C, d_out, oW, oH, homs, 1, **kw)

    cases = [
        (dict(d_out=p + 2 * (N * e - 1)), "overlap"), (dict(d_out=p), "overlap"),
        (dict(action=ACTIONS, out_slot=SLOTS, oW=W + 1), "COPY"),
        (dict(out_slot=[0, 1, 2, 1, 3]), "same slot"),
        (dict(out_slot=[0, 1, -1, 2, 3]), "below 0"),
        (dict(C=4), "nb_layers"),
    ]
    for kw, text in cases:
        rc = call(**kw)
        assert rc != 0 and text in gpu_ctx.error(), (kw, rc, gpu_ctx.error())
    torch.cuda.synchronize()
    assert np.array_equal(buf.cpu().numpy(), before)
    # the host entry refuses the same way
    out = np.full((N, 1, H, W), SENT, dtype=np.uint16)
    rc, _ = gpu_ctx.warp_frames(_frames(1), homs, (W, H), 1, out_slot=[0, 1, 2, 1, 3], out=out)
    assert rc != 0 and "same slot" in gpu_ctx.error() and (out == SENT).all()
    assert call() == 0
