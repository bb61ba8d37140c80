"""Automatic cosmetic correction on the device (sg_cosme_autodetect*) against the
literal restatement tests/cosme_ref.py (autodetect_literal): the corrected frames, icold / ihot,
status / failed_layer and the two statistics of every layer are equal exactly.  The cases are
tests/cosme_cases.py: planes with one dimension <= step, one tile - 1 / + 1 each way and two tiles
+ 1, odd widths, three layers with different statistics, chains longer than two tiles that cross
tile corners (horizontal, vertical, diagonal, a comb coupled through the 5 x 5 window; plain and
CFA), 5 % outliers of both signs, every parameter switch, the failure paths; plus a frame_stride
larger than the frame, a chunk + 1 frames through SG_COSME_CHUNK, a round list that overflows
(SG_COSME_LIST: the rounds walk the active plane instead), run-to-run identity and the host entry on
a batch that splits."""
import os

import numpy as np
import pytest

import cosme_cases as cc
import sirilgpu as sg

pytestmark = pytest.mark.gpu

GUARD = 0xABCD


def _device(ctx, frames, sig, amount, is_cfa, pad=0):
    """sg_cosme_autodetect_device on frames [N][C][H][W] with `pad` elements between frames; returns
    (rc, records, the frames as they come back); the gaps and the guard after them must not change"""
    import torch
    N, C, H, W = frames.shape
    stride = C * H * W + pad
    buf = np.full(N * stride + 64, GUARD, dtype=np.uint16)
    for f in range(N):
        buf[f * stride:f * stride + C * H * W] = frames[f].reshape(-1)
    d = torch.from_numpy(buf.view(np.int16).copy()).cuda()
    torch.cuda.synchronize()
    rc, rec = ctx.cosme_autodetect_device(d.data_ptr(), N, C, H, W, sig=sig, amount=amount, is_cfa=is_cfa,
                                          frame_stride=stride if pad else 0)
    torch.cuda.synchronize()
    back = d.cpu().numpy().view(np.uint16)
    out = np.stack([back[f * stride:f * stride + C * H * W].reshape(C, H, W) for f in range(N)])
    rest = np.ones(back.size, dtype=bool)
    for f in range(N):
        rest[f * stride:f * stride + C * H * W] = False
    assert (back[rest] == GUARD).all(), "the gap between frames or the guard changed"
    return rc, rec, out


def _compare(name, rec, out, label=None):
    label = label or name
    want = cc.literal_of(name)
    assert len(rec) == len(want)
    for f, (wout, wres) in enumerate(want):
        r = rec[f]
        got = {"status": r.status, "failed_layer": r.failed_layer, "icold": r.icold, "ihot": r.ihot,
               "bkg": list(r.bkg), "avg_dev": list(r.avg_dev)}
        print(f"cosme {label} f={f} got={got} diff={int((out[f] != wout).sum())}")
        assert got == wres, (label, f, got, wres)
        assert np.array_equal(out[f], wout), (label, f, np.argwhere(out[f] != wout)[:8].tolist())


@pytest.mark.parametrize("name", sorted(cc.CASES))
def test_equals_literal(gpu_ctx, name):
    c = cc.CASES[name]
    rc, rec, out = _device(gpu_ctx, cc.frames_of(name), c["sig"], c["amount"], c["is_cfa"])
    assert rc == 0, gpu_ctx.error()
    _compare(name, rec, out)


def test_cases_change_something():
    """the expectations are not vacuous: counts, changed pixels, truncation, the failure's layers"""
    for name in ("dense", "dense_cfa", "chain_comb", "layers3", "s_1x7", "s_2x9_cfa"):
        for fr, (wout, wres) in zip(cc.frames_of(name), cc.literal_of(name)):
            assert wres["icold"] + wres["ihot"] > 0 and not np.array_equal(fr, wout), name
    fr, (wout, wres) = cc.frames_of("amount_0")[0], cc.literal_of("amount_0")[0]
    assert wres["icold"] + wres["ihot"] > 0 and np.array_equal(fr, wout)
    fr, (wout, wres) = cc.frames_of("both_off")[0], cc.literal_of("both_off")[0]
    assert wres["icold"] + wres["ihot"] == 0 and np.array_equal(fr, wout)
    # 0.3: some corrected value has a fraction of at least 0.5, so rounding would differ
    a03, full = cc.literal_of("amount_03")[0][0], cc.literal_of("amount_05")[0][0]
    assert not np.array_equal(a03, full)
    fr, want = cc.frames_of("fail_layer1"), cc.literal_of("fail_layer1")
    assert [w[1]["status"] for w in want] == [0, 1, 0] and want[1][1]["failed_layer"] == 1
    assert not np.array_equal(want[1][0][0], fr[1, 0]) and np.array_equal(want[1][0][1:], fr[1, 1:])
    assert cc.literal_of("all_65535")[0][1]["bkg"][1] == 0.0


def test_frame_stride(gpu_ctx):
    c = cc.CASES["frames3"]
    rc, rec, out = _device(gpu_ctx, cc.frames_of("frames3"), c["sig"], c["amount"], c["is_cfa"], pad=37)
    assert rc == 0, gpu_ctx.error()
    _compare("frames3", rec, out, "stride")


def _with_chunk(chunk, fn, knob="SG_COSME_CHUNK"):
    """fn(ctx) on a context created under SG_COSME_CHUNK = chunk (the knobs are read once, at sg_init)"""
    old = os.environ.get(knob)
    os.environ[knob] = str(chunk)
    try:
        with sg.Context([0]) as ctx:
            return fn(ctx)
    finally:
        if old is None:
            del os.environ[knob]
        else:
            os.environ[knob] = old


@pytest.mark.parametrize("name", ["chain_comb", "dense_cfa", "fail_layer1"])
def test_list_overflow_walks_the_plane(gpu_ctx, name):
    """a round list of 8 entries: every round with more active pixels walks the active bit plane"""
    c = cc.CASES[name]

    def run(ctx):
        rc, rec, out = _device(ctx, cc.frames_of(name), c["sig"], c["amount"], c["is_cfa"])
        assert rc == 0, ctx.error()
        return rec, out, ctx.cosme_last_times()
    rec, out, times = _with_chunk(8, run, knob="SG_COSME_LIST")
    _compare(name, rec, out, name + " list 8")
    assert times[4] > 8 * times[3] > 0, times      # more pixels re-examined than the lists could hold


def test_chunk_plus_one_and_host_entry(gpu_ctx):
    """3 frames in chunks of 2 (+ 1): the device entry, and the host entry on a batch that splits"""
    for name in ("frames3", "fail_layer1"):
        c = cc.CASES[name]
        fr = cc.frames_of(name)

        def run(ctx):
            rc, rec, out = _device(ctx, fr, c["sig"], c["amount"], c["is_cfa"])
            assert rc == 0, ctx.error()
            host = fr.copy()
            rc, hrec = ctx.cosme_autodetect(host, sig=c["sig"], amount=c["amount"], is_cfa=c["is_cfa"])
            assert rc == 0, ctx.error()
            return rec, out, hrec, host
        rec, out, hrec, host = _with_chunk(2, run)
        _compare(name, rec, out, name + " chunk 2")
        _compare(name, hrec, host, name + " host")


def test_same_bits_twice(gpu_ctx):
    for name in ("dense", "chain_comb_cfa"):
        c = cc.CASES[name]
        runs = [_device(gpu_ctx, cc.frames_of(name), c["sig"], c["amount"], c["is_cfa"]) for _ in range(2)]
        assert runs[0][0] == 0 and runs[1][0] == 0
        assert runs[0][2].tobytes() == runs[1][2].tobytes()
        assert [bytes(r) for r in runs[0][1]] == [bytes(r) for r in runs[1][1]]


def test_chains_resolve_in_rounds(gpu_ctx):
    """the dependence is resolved by rounds over the listed pixels only: about as many rounds as the
    run is long, and far fewer pixels re-examined than rounds x image"""
    c = cc.CASES["chain_h"]
    fr = cc.frames_of("chain_h")
    rc, rec, out = _device(gpu_ctx, fr, c["sig"], c["amount"], c["is_cfa"])
    assert rc == 0, gpu_ctx.error()
    _, _, _, rounds, reexamined = gpu_ctx.cosme_last_times()
    print(f"cosme chain_h rounds={rounds} reexamined={reexamined} pixels={fr.size}")
    assert 100 <= rounds <= 160 and reexamined < 12 * fr.size // 10


REFUSED = [
    (dict(sig=(-0.5, 3.0)), sg.SG_ERR_GENERIC), (dict(sig=(3.0, float("nan"))), sg.SG_ERR_GENERIC),
    (dict(sig=(3.0, -2.0)), sg.SG_ERR_GENERIC), (dict(amount=1.5), sg.SG_ERR_GENERIC), (dict(amount=-0.1), sg.SG_ERR_GENERIC),
    (dict(amount=float("nan")), sg.SG_ERR_GENERIC), (dict(C=4), sg.SG_ERR_SIZE), (dict(C=0), sg.SG_ERR_SIZE),
    (dict(H=1, W=1), sg.SG_ERR_SIZE), (dict(H=2, W=2, is_cfa=True), sg.SG_ERR_SIZE), (dict(H=0), sg.SG_ERR_SIZE),
    (dict(N=0), sg.SG_ERR_SIZE), (dict(stride=5), sg.SG_ERR_SIZE),
]


@pytest.mark.parametrize("i", range(len(REFUSED)))
def test_refusals_leave_the_frames(gpu_ctx, i):
    import torch
    change, code = REFUSED[i]
    a = dict(N=1, C=1, H=4, W=6, sig=(3.0, 3.0), amount=1.0, is_cfa=False, stride=0)
    a.update(change)
    src = cc.frames_of("dense")[0, 0].reshape(-1)[:256].copy()
    d = torch.from_numpy(src.view(np.int16).copy()).cuda()
    torch.cuda.synchronize()
    rc, _ = gpu_ctx.cosme_autodetect_device(d.data_ptr(), a["N"], a["C"], a["H"], a["W"], sig=a["sig"], amount=a["amount"],
                                            is_cfa=a["is_cfa"], frame_stride=a["stride"])
    torch.cuda.synchronize()
    assert rc == code and gpu_ctx.error().startswith("cosme:"), (rc, gpu_ctx.error())
    assert np.array_equal(d.cpu().numpy().view(np.uint16), src)
