"""ECC registration on the device (sg_register_ecc_u16*) against the literal numpy
restatement tests/ecc_ref.py: iteration counts, failure flags and integer shifts equal, dx / dy / rho
within a measured bound, over shapes that cross every boundary of the kernels (one tile, W or H one
off a tile multiple, several tiles both ways), planted shifts that push the source tile out of the
image on every side, frames of one call that take different numbers of iterations, a pitched window
of a [3][H][W] sequence, `included` holes with ref_image != 0, a chunk + 1 frames call, the failure
paths, run-to-run bit identity and the host entry.

Measured on an MI355X over every case of this file against ecc_ref.ecc (literal form):
    max |dx - ref|, |dy - ref| = 7.153e-07 px,  max |rho - ref| / |ref| = 4.715e-08
(the kernel sums one-pass raw moments in fp64 where the literal form subtracts float means from float
planes; on the CPU the two forms differ by <= 4.8e-7 px on these scenes).  The bounds below are those
maxima times 4; independently dx / dy must agree within 2^-10 px, one step of the warp's coordinate
quantisation: a larger gap is a different algorithm, not rounding."""
import os

import numpy as np
import pytest

import ecc_ref as er
import sirilgpu as sg

pytestmark = pytest.mark.gpu

MEASURED_ABS = 7.153e-07    # px (see the header)
MEASURED_RHO = 4.715e-08    # relative
TOL_ABS = min(4 * MEASURED_ABS, 2.0 ** -10)
TOL_RHO = 4 * MEASURED_RHO
HARD_ABS = 2.0 ** -10
GUARD = 0xABCD

# 8 planted shifts, |s| <= 4, fractions from {.15, .25, .3, .7, .8}, both signs on both axes
SHIFTS = [(0.0, 0.0), (0.15, -0.25), (-1.3, 2.7), (2.8, -3.15), (-3.25, -1.7), (3.7, 3.3), (-0.8, 0.15), (1.25, -2.8),
          (-2.7, 3.8)]
# (H, W, seed): one tile; W, H off a tile multiple; tile height 32 - 1 / + 1; several tiles both ways
SHAPES = [(24, 32, 0), (37, 61, 1), (48, 64, 2), (63, 130, 3), (65, 257, 4), (31, 70, 5), (33, 70, 0)]

_frames = {}
_refs = {}
_worst = {"abs": 0.0, "rho": 0.0}


def frames_of(H, W, seed, ref_at=0):
    """the scene's 9 frames; the unmoved one (the reference frame of the call) at index ref_at"""
    if (H, W, seed, ref_at) not in _frames:
        fr = er.scene(H, W, seed, SHIFTS[1:ref_at + 1] + SHIFTS[:1] + SHIFTS[ref_at + 1:])
        fr.setflags(write=False)
        _frames[(H, W, seed, ref_at)] = fr
    return _frames[(H, W, seed, ref_at)]


def ref_of(key, frames, ref_image=0, included=None):
    """the restatement's answers, computed once per case"""
    if key not in _refs:
        _refs[key] = er.register(frames, ref_image, included)
    return _refs[key]


def _device(ctx, frames, layer=0, window=None, ref_image=0, included=None):
    """sg_register_ecc_u16_device on frames [N][C][H][W] read in place (window = (y0, x0, h, w) of the layer);
    the frames and the guard after them must come back untouched"""
    import torch
    N, C, H, W = frames.shape
    buf = np.full(frames.size + 64, GUARD, dtype=np.uint16)
    buf[:frames.size] = frames.reshape(-1)
    d = torch.from_numpy(buf.view(np.int16).copy()).cuda()
    torch.cuda.synchronize()
    y0, x0, h, w = window if window else (0, 0, H, W)
    base = d.data_ptr() + 2 * (layer * H * W + y0 * W + x0)
    rc, res = ctx.register_ecc_device(base, N, h, w, ref_image=ref_image, included=included, frame_pitch=C * H * W,
                                      row_pitch=W)
    torch.cuda.synchronize()
    assert np.array_equal(d.cpu().numpy().view(np.uint16), buf), "the frames or the guard changed"
    return rc, res


def _compare(res, want, label):
    """equal counts, flags and shifts; dx / dy / rho within the bound; the reference's values first"""
    for f, w in enumerate(want):
        if w is None:
            assert all(res[k][f] == 0 for k in res), (label, f, "a frame outside `included` was written")
            continue
        if not w["failed"] and w["iterations"] > 0:
            for v in (float(w["dx"]), float(w["dy"])):
                frac = abs(v - np.floor(v) - 0.5)
                assert frac >= 0.1, (label, f, v, "the reference's own value is too near a half-integer")
    for f, w in enumerate(want):
        if w is None:
            continue
        got = {k: res[k][f] for k in res}
        print(f"ecc {label} f={f} it={got['iterations']} failed={got['failed']} dx={got['dx']:.7f} dy={got['dy']:.7f} "
              f"rho={got['rho']:.9f} | ref it={w['iterations']} dx={float(w['dx']):.7f} dy={float(w['dy']):.7f} "
              f"rho={float(w['rho']):.9f}")
        assert (got["iterations"], got["failed"]) == (w["iterations"], w["failed"]), (label, f, got, w)
        assert (got["shiftx"], got["shifty"]) == (w["shiftx"], w["shifty"]), (label, f, got, w)
        if w["failed"]:
            assert (got["dx"], got["dy"], got["shiftx"], got["shifty"]) == (0, 0, 0, 0), (label, f, got)
            assert np.isnan(got["rho"]) == np.isnan(w["rho"]) and (np.isnan(w["rho"]) or got["rho"] == w["rho"])
            continue
        ea = max(abs(float(got["dx"]) - float(w["dx"])), abs(float(got["dy"]) - float(w["dy"])))
        er_ = abs(float(got["rho"]) - float(w["rho"])) / abs(float(w["rho"])) if w["rho"] != 0 else abs(float(got["rho"]))
        _worst["abs"], _worst["rho"] = max(_worst["abs"], ea), max(_worst["rho"], er_)
        print(f"ecc {label} f={f} err_abs={ea:.3e} err_rho={er_:.3e} worst_abs={_worst['abs']:.3e} worst_rho={_worst['rho']:.3e}")
        assert ea <= HARD_ABS, (label, f, ea, "beyond one step of the warp's quantisation: another algorithm")
        assert ea <= TOL_ABS and er_ <= TOL_RHO, (label, f, ea, er_)


def _same_bits(a, b):
    return all(a[k].tobytes() == b[k].tobytes() for k in a)


@pytest.mark.parametrize("H,W,seed", SHAPES)
def test_shapes_against_restatement(gpu_ctx, H, W, seed):
    fr = frames_of(H, W, seed)
    want = ref_of(("shape", H, W, seed), fr)
    its = [w["iterations"] for w in want[1:]]
    rc, res = _device(gpu_ctx, fr[:, None])
    assert rc == 0, gpu_ctx.error()
    assert (res["iterations"][0], res["shiftx"][0], res["shifty"][0], res["failed"][0]) == (0, 0, 0, 0)
    _compare(res, want, f"{H}x{W}")
    if (H, W) == (65, 257):
        assert len(set(its)) > 1, its   # frames of one launch grid finish at different iterations
    rc, again = _device(gpu_ctx, fr[:, None])
    assert rc == 0 and _same_bits(res, again), "two runs of the same call differ"
    rc, host = gpu_ctx.register_ecc(fr)
    assert rc == 0 and _same_bits(res, host), "the host entry differs from the device entry"


def test_pitched_window_of_a_three_layer_sequence(gpu_ctx):
    H, W, seed = 63, 130, 3
    a = frames_of(H, W, seed)
    seq = np.stack([np.flip(a, 1), a, np.flip(a, 2)], axis=1)   # [9][3][H][W], layer 1 is the scene
    y0, x0, h, w = 5, 17, 49, 97
    crop = np.ascontiguousarray(seq[:, 1, y0:y0 + h, x0:x0 + w])
    want = ref_of(("window", H, W, seed), crop)
    rc, res = _device(gpu_ctx, seq, layer=1, window=(y0, x0, h, w))
    assert rc == 0, gpu_ctx.error()
    _compare(res, want, "window")
    rc, host = gpu_ctx.register_ecc(seq, layer=1)
    assert rc == 0
    rc, whole = _device(gpu_ctx, seq, layer=1)
    assert rc == 0 and _same_bits(whole, host)
    _compare(whole, ref_of(("shape", H, W, seed), a), "layer1")


def test_included_holes_and_reference_not_first(gpu_ctx):
    H, W, seed = 48, 64, 2
    fr = frames_of(H, W, seed, ref_at=3)
    inc = np.array([1, 0, 1, 1, 0, 1, 1, 0, 1], dtype=np.int32)
    want = ref_of(("holes", H, W, seed), fr, 3, inc)
    rc, res = _device(gpu_ctx, fr[:, None], ref_image=3, included=inc)
    assert rc == 0, gpu_ctx.error()
    assert want[0] is not None and want[0]["iterations"] > 0 and want[1] is None
    _compare(res, want, "holes")
    rc, host = gpu_ctx.register_ecc(fr, ref_image=3, included=inc)
    assert rc == 0 and _same_bits(res, host)


def _with_chunk(chunk, fn):
    old = os.environ.get("SG_ECC_CHUNK")
    os.environ["SG_ECC_CHUNK"] = str(chunk)
    try:
        with sg.Context([0]) as ctx:
            return fn(ctx)
    finally:
        if old is None:
            del os.environ["SG_ECC_CHUNK"]
        else:
            os.environ["SG_ECC_CHUNK"] = old


@pytest.mark.parametrize("chunk", [8, 2])
def test_chunk_plus_one_frames(gpu_ctx, chunk):
    """9 frames in chunks of 8 (+ 1) and of 2: the same bits as one chunk; reference in another chunk than its frames"""
    H, W, seed = 37, 61, 1
    fr = frames_of(H, W, seed, ref_at=4)
    rc, one = _device(gpu_ctx, fr[:, None], ref_image=4)
    assert rc == 0, gpu_ctx.error()
    _compare(one, ref_of(("chunk", H, W, seed), fr, 4), "chunk")

    def run(ctx):
        rc, dev = _device(ctx, fr[:, None], ref_image=4)
        assert rc == 0, ctx.error()
        rc, host = ctx.register_ecc(fr, ref_image=4)
        assert rc == 0, ctx.error()
        return dev, host
    dev, host = _with_chunk(chunk, run)
    assert _same_bits(one, dev) and _same_bits(one, host)


def test_failure_paths_leave_the_other_frames_alone(gpu_ctx):
    """an all-zero frame, a x100 frame (constant 255 after the clamp) and the 24 x 32 scene moved by (4.7, -4.2)
    (seed 1 of ecc_ref.scene ends with rho = -1; seed 7, which converges there, rides along)"""
    H, W = 24, 32
    a = er.scene(H, W, 1, [(0, 0), (1.3, -0.7), (4.7, -4.2), (-2.25, 1.8)])
    b = er.scene(H, W, 7, [(0, 0), (4.7, -4.2)])
    x100 = (a[0].astype(np.uint32) * 100).clip(0, 65535).astype(np.uint16)
    fr = np.stack([a[0], a[1], np.zeros_like(a[0]), x100, a[2], a[3]])
    want = ref_of(("fail", 1), fr)
    assert [w["failed"] for w in want] == [0, 0, 1, 1, 1, 0] and want[4]["rho"] == -1.0
    rc, res = _device(gpu_ctx, fr[:, None])
    assert rc == 0, gpu_ctx.error()
    _compare(res, want, "fail")
    clean = np.stack([a[0], a[1], a[3]])
    rc, alone = _device(gpu_ctx, clean[:, None])
    assert rc == 0
    for k in res:   # the good frames: the same bits with and without the failing neighbours
        assert res[k][[0, 1, 5]].tobytes() == alone[k].tobytes(), k
    rc, res7 = _device(gpu_ctx, b[:, None])
    assert rc == 0
    _compare(res7, ref_of(("fail", 7), b), "seed7")
    rc, host = gpu_ctx.register_ecc(fr)
    assert rc == 0 and _same_bits(res, host)


def test_clamp_on_the_device(gpu_ctx):
    H, W, seed = 37, 61, 1
    fr = frames_of(H, W, seed)[:3].copy()
    hot = fr.copy()
    hot[fr > 200] = 60000
    rc, a = _device(gpu_ctx, np.minimum(hot, 255)[:, None])
    rc2, b = _device(gpu_ctx, hot[:, None])
    assert rc == 0 and rc2 == 0 and _same_bits(a, b) and (a["failed"] == 0).all()


def test_refused_arguments(gpu_ctx):
    fr = frames_of(24, 32, 0)
    import torch
    d = torch.from_numpy(fr.view(np.int16).copy()).cuda()
    for kw, h, w in [({}, 7, 32), ({}, 24, 7), ({"ref_image": 9}, 24, 32), ({"ref_image": -1}, 24, 32),
                     ({"row_pitch": 31}, 24, 32), ({"frame_pitch": 24 * 32 - 1}, 24, 32)]:
        rc, _ = gpu_ctx.register_ecc_device(d.data_ptr(), 9, h, w, **kw)
        assert rc == sg.SG_ERR_SIZE, (kw, h, w, rc)
        assert "ecc:" in gpu_ctx.error()
    rc, _ = gpu_ctx.register_ecc_device(0, 9, 24, 32)
    assert rc == sg.SG_ERR_GENERIC
