"""One-star registration on the device (sg_seqpsf_u16*, sg_seqpsf_shifts) against the numpy restatement
tests/seqpsf_ref.py over its CASES (tests/test_seqpsf_cpu.py holds what they rely on): the integer and exact
fields (status, angle_fitted, both iteration counts, the clamped area, ngood, bg, the start values, the
shifts) equal for every frame, the fp fields within seqpsf_ref.TOL on branch-stable frames, NaN matching
NaN.  Shapes (15 x 11 and 11 x 15 on one star, 7 x 1, 1 x 7, 3 x 2, 7 x 5 below one wave, 128 x 128 with two
equal maxima more than 4096 pixels apart, 129 x 8 refused), the angle (+30 and -60 degrees, a round star,
fit_angle = 0), the background (mostly zero, saturated, blank), clamping at every side and corner,
REGISTERED framing, four FOLLOW_STAR chains with skipped frames, a pitched layer of [3][H][W] frames, a
caller's stream, run-to-run bits and the host entry in batches of 2."""
import os

import numpy as np
import pytest

import seqpsf_ref as sr
import sirilgpu as sg
from test_seqpsf_cpu import check_record

pytestmark = pytest.mark.gpu

GUARD = 0xABCD


def _device(ctx, frames, area, layer=0, C=1, pad=0, stream=None, **kw):
    """sg_seqpsf_u16_device on frames [N][H][W] placed as layer `layer` of [N][C][H][W + pad] frames read in
    place; the buffer and the guard after it must come back untouched"""
    import torch
    N, H, W = frames.shape
    rp = W + pad
    full = np.full((N, C, H, rp), 0x1234, dtype=np.uint16)
    full[:, layer, :, :W] = frames
    buf = np.full(full.size + 64, GUARD, dtype=np.uint16)
    buf[:full.size] = full.reshape(-1)
    d = torch.from_numpy(buf.view(np.int16).copy()).cuda()
    torch.cuda.synchronize()
    rc, rec, carry = ctx.seqpsf_device(d.data_ptr() + 2 * layer * H * rp, N, H, W, area, frame_pitch=C * H * rp, row_pitch=rp,
                                       stream=stream, **kw)
    torch.cuda.synchronize()
    assert np.array_equal(d.cpu().numpy().view(np.uint16), buf), "the frames or the guard changed"
    return rc, rec, carry


def _args(c):
    a = dict(c["args"])
    return dict(framing=a.get("framing", sr.ORIGINAL), included=a.get("included"), reg_shifts=a.get("reg_shifts"),
                fit_angle=a.get("fit_angle", True))


def _compare(name, rec, carry, c):
    assert len(rec) == len(c["records"])
    for f, w in enumerate(c["records"]):
        g = rec[f]
        print(name, f, "status", g["status"], "iters", g["iters"], g["iters_angle"], "area", g["area_x"], g["area_y"], "bg", g["bg"],
              "fwhm", g["fwhmx"], g["fwhmy"], "angle", g["angle"], "| ref", w["status"], w["iters"], w["iters_angle"],
              float(w["fwhmx"]), float(w["fwhmy"]), float(w["angle"]), "stable", bool(c["stable"][f]))
        check_record(g, w, bool(c["stable"][f]), where=(name, f))
    assert tuple(carry) == tuple(c["carry"]), (name, carry, c["carry"])
    rc, sx, sy, fw, best, bf = sg.seqpsf_shifts(rec, 0)
    wrc, wsx, wsy, wfw, wbest, wbf = c["shifts"]
    assert rc == wrc, (name, rc, wrc)
    if rc == 0:
        assert sx.tolist() == wsx.tolist() and sy.tolist() == wsy.tolist() and best == wbest, (name, sx, wsx, sy, wsy, best, wbest)
        assert np.array_equal(fw, rec["fwhmx"] * (rec["status"] == 0)) and bf == fw[best]


@pytest.mark.parametrize("name", list(sr.CASES))
def test_case(gpu_ctx, name):
    c = sr.case(name)
    rc, rec, carry = _device(gpu_ctx, c["frames"], c["area"], **_args(c))
    assert rc == 0, gpu_ctx.error()
    _compare(name, rec, carry, c)


def test_shapes_differ_and_agree(gpu_ctx):
    """15 x 11 and 11 x 15 on the same star: the same star position and shape from two boxes (a transposed or
    swapped index would move it), not the same bits"""
    a, b = sr.case("a15x11"), sr.case("a11x15")
    ra = _device(gpu_ctx, a["frames"], a["area"])[1]
    rb = _device(gpu_ctx, b["frames"], b["area"])[1]
    for f in range(len(ra)):
        assert abs(ra[f]["xpos"] - rb[f]["xpos"]) < 0.05 and abs(ra[f]["ypos"] - rb[f]["ypos"]) < 0.05
        assert abs(ra[f]["angle"] - rb[f]["angle"]) < 1.0 and ra[f]["x0"] != rb[f]["x0"]


def test_refused(gpu_ctx):
    fr = sr.case("plus30")["frames"]
    for area, kw, code in (((10, 10, 129, 8), {}, -2), ((10, 10, 0, 8), {}, -2), ((0, 0, 65, 8), {}, -2),
                           ((10, 10, 15, 15), dict(framing=3), -1), ((10, 10, 15, 15), dict(framing=sr.REGISTERED), -1),
                           ((10, 10, 15, 15), dict(norm=255.0), -1), ((10, 10, 15, 15), dict(scales=(float("nan"), 1.0)), -1)):
        rc, rec, _ = _device(gpu_ctx, fr, area, **kw)
        assert rc == code and gpu_ctx.error(), (area, kw, rc)
        assert not rec["status"].any() and not rec["ngood"].any()       # nothing written


def test_noangle_is_step_4_alone(gpu_ctx):
    c = sr.case("plus30")
    r1 = _device(gpu_ctx, c["frames"], c["area"])[1]
    r0 = _device(gpu_ctx, c["frames"], c["area"], fit_angle=False)[1]
    assert r0["noangle"].tobytes() == r1["noangle"].tobytes() and r0["init"].tobytes() == r1["init"].tobytes()
    assert not r0["angle_fitted"].any() and r1["angle_fitted"].all() and not r0["angle"].any()
    assert np.array_equal(r0["sx"], r0["noangle"][:, 4]) and np.array_equal(r0["B"], r0["noangle"][:, 0] / 65535.0)


def test_follow_differs_from_original_and_static_chain_equals_it(gpu_ctx):
    d0, d1 = sr.case("drift_original"), sr.case("drift_follow")
    r0 = _device(gpu_ctx, d0["frames"], d0["area"], **_args(d0))[1]
    r1 = _device(gpu_ctx, d1["frames"], d1["area"], **_args(d1))[1]
    assert r0[8]["status"] != 0 and r1[8]["status"] == 0 and r1[8]["area_x"] != r0[8]["area_x"]
    s0, s1 = sr.case("static_original"), sr.case("static_follow")
    a = _device(gpu_ctx, s0["frames"], s0["area"], **_args(s0))[1]
    b = _device(gpu_ctx, s1["frames"], s1["area"], **_args(s1))[1]
    assert a.tobytes() == b.tobytes()


def test_layer_pitch_stream_and_same_bits(gpu_ctx):
    """layer 1 of [3][H][W + 5] frames, on a caller's stream; two runs give the same bits as the tight run"""
    import torch
    for name in ("plus30", "drift_follow"):
        c = sr.case(name)
        tight = _device(gpu_ctx, c["frames"], c["area"], **_args(c))
        s = torch.cuda.Stream()
        runs = [_device(gpu_ctx, c["frames"], c["area"], layer=1, C=3, pad=5, stream=s.cuda_stream, **_args(c)) for _ in range(2)]
        for rc, rec, carry in runs:
            assert rc == 0 and rec.tobytes() == tight[1].tobytes() and carry == tight[2]
        _compare(name, runs[0][1], runs[0][2], c)


def test_carry_enters_the_chain(gpu_ctx):
    """a chain started from a carried area equals the tail of the whole chain"""
    c = sr.case("drift_follow")
    whole = _device(gpu_ctx, c["frames"], c["area"], **_args(c))
    head = _device(gpu_ctx, c["frames"][:4], c["area"], framing=sr.FOLLOW_STAR, included=sr.SKIP_1[:4])
    tail = _device(gpu_ctx, c["frames"][4:], c["area"], framing=sr.FOLLOW_STAR, included=sr.SKIP_1[4:], carry=head[2])
    assert head[1].tobytes() + tail[1].tobytes() == whole[1].tobytes() and tail[2] == whole[2]


def _context(**env):
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


def test_host_entry_in_batches(gpu_ctx):
    """SG_HOST_BATCH=2 over 5 frames, FOLLOW_STAR (one chain that runs through, one stopped in batch 1) and
    ORIGINAL: the same bits as one batch and as the device entry; last_times reports the batches' launches"""
    ctx2 = _context(SG_HOST_BATCH=2)
    try:
        for name, launches in (("drift_follow", 3), ("plus30", 3), ("blankmid_follow", 3)):
            c = sr.case(name)
            a = _args(c)
            fr = c["frames"][:5] if name != "blankmid_follow" else c["frames"][2:7]     # blank at index 2: batch 1
            inc = None if a["included"] is None else (a["included"][:5] if name != "blankmid_follow" else a["included"][2:7])
            kw = dict(a, included=inc)
            dev = _device(gpu_ctx, fr, c["area"], **kw)
            one = gpu_ctx.seqpsf(fr, c["area"], **kw)
            two = ctx2.seqpsf(fr, c["area"], **kw)
            assert one[0] == 0 and two[0] == 0, (gpu_ctx.error(), ctx2.error())
            assert one[1].tobytes() == dev[1].tobytes() == two[1].tobytes() and one[2] == dev[2] == two[2], name
            assert gpu_ctx.seqpsf_last_times()[1] == 1
            ms, n = ctx2.seqpsf_last_times()
            if name == "blankmid_follow":
                assert two[1]["status"].tolist() == [0, 0, sr.FIT_NONFINITE, sr.NOT_RUN, sr.NOT_RUN] and n == 2   # batch 2 not launched
                assert sg.seqpsf_shifts(two[1])[0] == 1
            else:
                assert n == launches and ms > 0
        # host frames [N][C][H][W], another layer
        c = sr.case("plus30")
        st = np.stack([c["frames"] // 2, c["frames"], c["frames"] // 3], axis=1)
        rc, rec, _ = ctx2.seqpsf(st, c["area"], layer=1)
        assert rc == 0 and rec.tobytes() == _device(gpu_ctx, c["frames"], c["area"])[1].tobytes()
    finally:
        ctx2.close()


def test_shifts_returns(gpu_ctx):
    c = sr.case("drift_follow")
    rec = _device(gpu_ctx, c["frames"], c["area"], **_args(c))[1]
    assert sg.seqpsf_shifts(rec, 1)[0] == -1           # frame 1 is excluded
    rc, sx, sy, fw, best, bf = sg.seqpsf_shifts(rec, 2)
    w = sr.shifts(c["records"], 2)
    assert rc == 0 and sx.tolist() == w[1].tolist() and sy.tolist() == w[2].tolist() and best == w[4]
