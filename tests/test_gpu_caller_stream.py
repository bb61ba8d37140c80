"""Every *_device entry on a stream of the caller's whose producer is still running when the entry is
called.  The input buffer holds zeros; on the caller's stream a delay and then a device-to-device copy
of the real frames are queued, and the entry is called with that stream while the delay runs.  An
entry that read its input from any other stream (an internal copy, memset or auxiliary kernel left on
the library's own stream) would see the zero frames, which are valid data with another answer, so the
usual comparison with the reference fails; nothing can fault.  A warm-up call of the same shape on the
same stream comes first, so that the tested call allocates and frees nothing (a free would wait for
the device and hide the race).

The delay is torch.cuda._sleep(SLEEP_CYCLES): 41.6 ms on an MI355X for 10^8 cycles, measured with torch
events (12.5 ms for 3 x 10^7, 4.2 ms for 10^7).  Each case waits for it once."""
import numpy as np
import pytest

import findstar_ref as fr
import oracle_lib as orc
import prepro_ref as ppr
import psf_ref as pr
import sirilgpu as sg
import warp_ref
from test_gpu_prepro import _fit, _noise_frame, KS
from test_gpu_register import _same_q
from test_gpu_starfit import _check_frame
from test_gpu_stats import _frames as _stats_frames
from test_warp import _img

pytestmark = pytest.mark.gpu

SLEEP_CYCLES = 10 ** 8


class _Late:
    """a device buffer whose content arrives late on a stream of its own"""

    def __init__(self, data):
        import torch
        self.torch = torch
        self.host = np.ascontiguousarray(data, dtype=np.uint16).reshape(-1)
        self.src = torch.from_numpy(self.host.view(np.int16).copy()).cuda()
        self.buf = self.src.clone()
        self.s = torch.cuda.Stream()
        self.stream = self.s.cuda_stream
        assert self.stream != 0
        torch.cuda.synchronize()

    def ptr(self):
        return self.buf.data_ptr()

    def arm(self):
        """zeros now; the real content after the delay, on the stream"""
        torch = self.torch
        torch.cuda.synchronize()
        self.buf.zero_()
        torch.cuda.synchronize()
        with torch.cuda.stream(self.s):
            torch.cuda._sleep(SLEEP_CYCLES)
            self.buf.copy_(self.src, non_blocking=True)
        assert not self.s.query(), "the producer had finished before the call: the case proves nothing"

    def read(self, t=None):
        self.s.synchronize()
        self.torch.cuda.synchronize()
        return (self.buf if t is None else t).cpu().numpy().view(np.uint16)


def _late_call(late, call, out=None):
    """warm-up on the stream, then the call under test with the input still on its way (and the device
    output, if any, zero again)"""
    call()
    if out is not None:
        late.s.synchronize()
        out.zero_()
    late.arm()
    return call()


def test_findstar_fit_device(gpu_ctx):
    img = pr.starfit_frame(5)
    H, W = img.shape
    late = _Late(img)
    rc, rec, nstars, st, cd = _late_call(late, lambda: gpu_ctx.findstar_fit_device(
        late.ptr(), 1, 1, H, W, 5, pr.K_SIGMA, max_candidates=64, max_stars=64, want_candidates=True, stream=late.stream))
    assert rc == 0, gpu_ctx.error()
    assert rec[0].no_data == 0 and nstars[0] >= 10
    _check_frame(img, rec[0], nstars[0], st[0], cd[0], 5)
    assert np.array_equal(late.read(), late.host)


def test_findstar_device(gpu_ctx):
    import torch
    img, r = fr.star_case(0)
    H, W = img.shape
    late = _Late(img)
    dw = torch.zeros(H * W, dtype=torch.int16, device="cuda")
    rc, rec, xy, bx = _late_call(late, lambda: gpu_ctx.findstar_device(
        late.ptr(), 1, 1, H, W, r, 1.0, max_candidates=64, d_wave=dw.data_ptr(), stream=late.stream), out=dw)
    assert rc == 0, gpu_ctx.error()
    cands, want, wave = fr.candidates(img, 1.0, r)
    n = len(cands)
    assert 2 <= n <= 64 and rec[0].ncand == n and rec[0].no_data == 0
    assert rec[0].ngood == want["ngood"] and rec[0].threshold == want["threshold"]
    assert xy[0, :n].tolist() == [list(c) for c in cands] and np.array_equal(bx[0, :n], fr.boxes(img, cands, r))
    assert np.array_equal(late.read(dw).reshape(H, W), wave)


def _prepro_case():
    frames, dark, k_ref = _fit(9, 67)
    off = np.random.default_rng(5).integers(90, 110, size=(1, 9, 67)).astype(np.uint16)
    kw = dict(offset=off, dark=dark[None], dark_optimization=True, cosmetic=True, cosme_sigma=(3.0, 3.0))
    return frames, kw, k_ref


def test_prepro_frames_device(gpu_ctx):
    """in place: the warm-up calibrates the buffer, the late copy then brings the raw frames again"""
    frames, kw, k_ref = _prepro_case()
    want, _ = ppr.preprocess(frames, **kw)
    late = _Late(frames)
    with sg.Prepro(gpu_ctx, 67, 9, 1, **kw) as pp:
        rc, k = _late_call(late, lambda: gpu_ctx.prepro_frames_device(pp, late.ptr(), frames.shape[0], stream=late.stream))
        assert rc == 0, gpu_ctx.error()
        got = late.read().reshape(frames.shape)
    assert k.tobytes() == k_ref.tobytes(), (k, k_ref)
    assert np.array_equal(got, want), np.argwhere(got != want)[:5]


def test_prepro_noise_device(gpu_ctx):
    raw, dark = _noise_frame(np.random.default_rng(129), 8, 129)
    frames = np.stack([raw] * len(KS))[:, None]
    late = _Late(frames)
    with sg.Prepro(gpu_ctx, 129, 8, 1, dark=dark) as pp:
        rc, noise = _late_call(late, lambda: gpu_ctx.prepro_noise_device(pp, late.ptr(), len(KS), KS, stream=late.stream))
    assert rc == 0, gpu_ctx.error()
    for i, k in enumerate(KS):
        want = ppr.objective(raw, dark, k)
        assert np.float64(noise[i]).tobytes() == np.float64(want).tobytes() and want > 0.0, (k, noise[i], want)
    assert np.array_equal(late.read(), late.host)


def test_frame_stats_ikss_device(gpu_ctx):
    frames = _stats_frames()
    N, C, H, W = frames.shape
    late = _Late(frames)
    rc, loc, scl = _late_call(late, lambda: gpu_ctx.frame_stats_ikss(late.ptr(), N, C, H, W, stream=late.stream))
    assert rc == 0, gpu_ctx.error()             # the zero frames would be refused as empty
    for i in range(N):
        orc_rc, l, s = orc.statistics_ikss(frames[i])
        assert orc_rc == 0 and loc[i] == l and scl[i] == s, (i, loc[i], l, scl[i], s)


def test_register_dft_u16_device(gpu_ctx):
    S, n = 64, 6
    sel = orc.synth(n, 1, S, S, seed=9, maxshift=5)[:, 0].copy()        # the selections of smoke()
    late = _Late(sel)
    gx, gy, gq = _late_call(late, lambda: gpu_ctx.register_dft_device(late.ptr(), n, S, stream=late.stream))
    rx, ry, rq = orc.register_dft(sel)
    assert rx.any() or ry.any()                 # identical (zero) frames would register at (0, 0)
    assert np.array_equal(gx, rx) and np.array_equal(gy, ry), (gx, rx, gy, ry)
    assert _same_q(gq, rq), (gq, rq)


def test_stack_u16_device(gpu_ctx):
    import torch
    N, C, H, W = 12, 1, 40, 70
    frames = orc.synth(N, C, H, W, seed=21, maxshift=0)
    rc, ref, rej_ref = orc.stack_rejection(frames, sg.SIGMA, sig=(3.0, 3.0), max_thread=4)
    assert rc == 0 and ref.any()
    late = _Late(frames)
    o = torch.zeros(C * H * W, dtype=torch.int16, device="cuda")
    desc, keep = sg.make_desc(sg.MEAN, N, W, H, C, rejection=sg.SIGMA, sig=(3.0, 3.0), max_thread=4, max_number_of_rows=H)

    rej, _ = _late_call(late, lambda: gpu_ctx.stack_device(desc, late.ptr(), C * H * W, H * W, o.data_ptr(), 0, H,
                                                           stream=late.stream), out=o)
    assert np.array_equal(late.read(o).reshape(C, H, W), ref)
    assert np.array_equal(rej, rej_ref)


@pytest.mark.parametrize("interp", [0, 1, 2, 3, 4])
def test_warp_u16_device(gpu_ctx, interp):
    """given a stream the entry returns with the kernel queued: the result is read by a copy queued on the
    same stream after the call.  Without a stream it waits itself."""
    import torch
    C, H, W, oW, oH = 3, 57, 83, 92, 52
    img = _img(C, H, W, interp)
    hom = np.array([[np.cos(0.04), -np.sin(0.04), 2.7], [np.sin(0.04), np.cos(0.04), -3.1], [1.5e-4, -1e-4, 1.0]])
    exp = warp_ref.warp(img, hom, (oW, oH), interp)
    assert exp.any()
    late = _Late(img)
    out = torch.zeros(C * oH * oW, dtype=torch.int16, device="cuda")
    keep = torch.zeros_like(out)

    def call():
        gpu_ctx.warp_device(late.ptr(), W, H, C, out.data_ptr(), oW, oH, hom, interp, stream=late.stream)

    _late_call(late, call, out=out)
    with torch.cuda.stream(late.s):
        keep.copy_(out, non_blocking=True)
    got = late.read(keep).reshape(C, oH, oW)
    assert np.array_equal(got, exp), np.argwhere(got != exp)[:5]
    # the library's own stream: the call waits for the kernel
    out.zero_()
    torch.cuda.synchronize()
    gpu_ctx.warp_device(late.ptr(), W, H, C, out.data_ptr(), oW, oH, hom, interp)
    got = out.cpu().numpy().view(np.uint16).reshape(C, oH, oW)
    assert np.array_equal(got, exp), np.argwhere(got != exp)[:5]
