"""QualityEstimate of whole layers on the device (sg_quality_u16*) against
oracle_lib.quality (oracle/or_registration.c: or_quality_estimate): equal bit for bit, NaN matching
NaN, under the resident route and under the tiled route (contexts made with SG_QUALITY_ROUTE).  The
shapes and contents are tests/quality_cases.py: planes without samples (0.0, nothing launched),
planes whose margins leave no row (NaN), the smallest interior, every remainder of W - 1 and H - 1
mod 3, 63 .. 66 samples across, one sample fewer and one more than each tile dimension both ways,
640 x 480 once; all-zero, constant, saturated, clamping and sparse-map frames.  Then the layouts and
calls: a layer of three, a pitched window with an odd origin, the frames and a guard unchanged,
`included` with holes, chunks through SG_QUALITY_CHUNK, the route boundary moved by SG_QUALITY_LDS,
run-to-run identity, the host entry, register_ecc's whole glue, and every refusal."""
import os

import numpy as np
import pytest

import ecc_ref as er
import oracle_lib as orc
import quality_cases as qc
import sirilgpu as sg

pytestmark = pytest.mark.gpu

GUARD = 0xABCD
SENTINEL = -12345.5
NONE, RESIDENT, TILED = 0, 1, 2
ROUTES = [RESIDENT, TILED]
_want = {}


def want_of(key, planes):
    """the oracle's values of the planes [N][H][W], computed once per key"""
    if key not in _want:
        _want[key] = np.array([orc.quality(p) for p in planes], dtype=np.float64)
    return _want[key]


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
def ctxs(gpu_ctx):
    c = {r: _context(SG_QUALITY_ROUTE=r) for r in ROUTES}
    yield c
    for x in c.values():
        x.close()


def _device(ctx, frames, layer=0, window=None, included=None):
    """sg_quality_u16_device on layer `layer` of frames [N][C][H][W] (window = (y0, x0, h, w) inside it), read
    in place; returns (rc, quality_raw with SENTINEL where nothing was written); the buffer and a guard after
    it must come back unchanged"""
    import torch
    N, C, H, W = frames.shape
    y0, x0, h, w = window or (0, 0, H, W)
    buf = np.concatenate([frames.reshape(-1), np.full(64, GUARD, dtype=np.uint16)])
    d = torch.from_numpy(buf.view(np.int16).copy()).cuda()
    torch.cuda.synchronize()
    base = d.data_ptr() + 2 * (layer * H * W + y0 * W + x0)
    rc, q = ctx.quality_device(base, N, h, w, included=included, frame_pitch=C * H * W, row_pitch=W, fill=SENTINEL)
    torch.cuda.synchronize()
    assert np.array_equal(d.cpu().numpy().view(np.uint16), buf), "the frames or the guard changed"
    return rc, q


def _check(label, got, want):
    print(f"quality {label} got={got.tolist()} want={np.asarray(want).tolist()}")
    assert qc.same(got, want), (label, got.tolist(), np.asarray(want).tolist())


ALL_SHAPES = qc.SHAPES_ZERO + qc.SHAPES_NAN + qc.SHAPES + qc.SHAPES_TILE


@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("H, W", ALL_SHAPES)
def test_shapes_equal_the_oracle(ctxs, route, H, W):
    fr = qc.shape_frames(H, W)
    want = want_of((H, W), fr)
    rc, q = _device(ctxs[route], fr[:, None])
    assert rc == 0, ctxs[route].error()
    _check((H, W, route), q, want)
    ms, took, launches = ctxs[route].quality_last_times()
    if (H, W) in qc.SHAPES_ZERO:
        assert (took, launches) == (NONE, 0) and (q == 0.0).all()
    else:
        assert (took, launches) == (route, 1 if route == RESIDENT else 3)
        if (H, W) in qc.SHAPES_NAN:
            assert np.isnan(q).all()
        else:
            assert np.isfinite(q).all() and (q > 0).all()


@pytest.mark.parametrize("route", ROUTES + [0])
def test_planetary_frame(gpu_ctx, ctxs, route):
    """640 x 480: the largest shape of the suite, 213 x 159 samples; route 0 is the context's default"""
    H, W = qc.SHAPE_BIG
    fr = qc.shape_frames(H, W)
    ctx = ctxs[route] if route else gpu_ctx
    rc, q = _device(ctx, fr[:, None])
    assert rc == 0, ctx.error()
    _check((H, W, route), q, want_of((H, W), fr))
    assert q[0] == qc.GENERATOR_CHECKS[2][2]
    assert ctx.quality_last_times()[1] == (route or DEFAULT_ROUTE_640x480)


# the plan's choice for a 640 x 480 frame (DESIGN §2 records the measurement behind it)
DEFAULT_ROUTE_640x480 = RESIDENT


@pytest.mark.parametrize("route", ROUTES)
def test_contents_in_one_call(ctxs, route):
    """frames of different content in one call: all zero (NaN, no stretch), constants (0.0; 65535 leaves the
    maximum 0), a background above the maximum's limit, rows that make the stretch clamp, and the sparse maps of
    a 6 x 6 block at every position the margins and the dilation distinguish"""
    names = sorted(qc.CONTENT)
    fr = np.stack([qc.CONTENT[n][0] for n in names])
    want = want_of("content", fr)
    assert qc.same(want, [qc.CONTENT[n][1] for n in names])       # the values the cases were chosen for
    rc, q = _device(ctxs[route], fr[:, None])
    assert rc == 0, ctxs[route].error()
    _check(("content", route), q, want)


@pytest.mark.parametrize("route", ROUTES)
def test_layer_of_three_and_pitched_window(ctxs, route):
    H, W = 61, 75
    fr = np.stack([np.stack([qc.planet(H, W, 3 * f + c + 1, amp=300 * (c + 1) * (f + 1)) for c in range(3)]) for f in range(3)])
    rc, q = _device(ctxs[route], fr, layer=1)
    assert rc == 0, ctxs[route].error()
    _check(("layer 1", route), q, want_of("layer1", fr[:, 1]))
    assert not qc.same(q, want_of("layer0", fr[:, 0]))
    # an odd x0 and an odd row pitch, an odd base address in elements
    win = (5, 7, 37, 61)
    rc, q = _device(ctxs[route], fr, layer=2, window=win)
    assert rc == 0, ctxs[route].error()
    _check(("window", route), q, want_of("window", [np.ascontiguousarray(fr[f, 2, 5:5 + 37, 7:7 + 61]) for f in range(3)]))
    # rows that start on dwords (the dword loads) but are longer than the window: even x0 and pitch, an odd width
    ev = np.stack([qc.planet(40, 76, s, amp=30000) for s in (4, 5)])[:, None]
    rc, q = _device(ctxs[route], ev, window=(4, 6, 31, 47))
    assert rc == 0, ctxs[route].error()
    _check(("window even", route), q, want_of("window_even", [np.ascontiguousarray(ev[f, 0, 4:4 + 31, 6:6 + 47]) for f in range(2)]))


def _seven():
    return np.stack([qc.planet(37, 61, s, amp=200 + 37 * s) for s in range(1, 8)])


@pytest.mark.parametrize("route", ROUTES)
def test_included_holes_keep_the_sentinel(ctxs, route):
    fr = _seven()
    want = want_of("seven", fr)
    inc = np.array([0, 1, 1, 0, 0, 1, 0], dtype=np.int32)
    rc, q = _device(ctxs[route], fr[:, None], included=inc)
    assert rc == 0, ctxs[route].error()
    assert (q[inc == 0] == SENTINEL).all()
    _check(("holes", route), q[inc == 1], want[inc == 1])
    rc, q = _device(ctxs[route], fr[:, None], included=np.zeros(7, dtype=np.int32))
    assert rc == 0 and (q == SENTINEL).all() and ctxs[route].quality_last_times()[2] == 0


@pytest.mark.parametrize("route", ROUTES)
def test_five_frames_in_chunks_of_two(gpu_ctx, route):
    fr = _seven()[:5]
    want = want_of("seven", _seven())[:5]
    ctx = _context(SG_QUALITY_ROUTE=route, SG_QUALITY_CHUNK=2)
    try:
        rc, q = _device(ctx, fr[:, None])
        assert rc == 0, ctx.error()
        _check(("chunk 2", route), q, want)
        assert ctx.quality_last_times()[1:] == (route, 3 if route == RESIDENT else 9)
        rc, q = _device(ctx, fr[:, None], included=np.array([1, 0, 1, 1, 0], dtype=np.int32))
        assert rc == 0 and ctx.quality_last_times()[2] == (2 if route == RESIDENT else 6)
        _check(("chunk 2 holes", route), q[[0, 2, 3]], want[[0, 2, 3]])
        rc, q = ctx.quality(fr)         # the host entry's batches follow the knob too
        assert rc == 0, ctx.error()
        _check(("chunk 2 host", route), q, want)
    finally:
        ctx.close()


def test_lds_budget_moves_the_route_boundary(gpu_ctx):
    """SG_QUALITY_LDS = 320 bytes: 24 x 32 (70 samples, 320 bytes) is the last resident shape, 31 x 47 (150
    samples) the first tiled one under the plan's own choice"""
    ctx = _context(SG_QUALITY_LDS=320)
    try:
        for (H, W), route in (((24, 32), RESIDENT), ((31, 47), TILED)):
            fr = qc.shape_frames(H, W)
            rc, q = _device(ctx, fr[:, None])
            assert rc == 0, ctx.error()
            _check((H, W, "lds 320"), q, want_of((H, W), fr))
            assert ctx.quality_last_times()[1] == route, (H, W)
    finally:
        ctx.close()


@pytest.mark.parametrize("route", ROUTES)
def test_same_bits_twice(ctxs, route):
    fr = qc.shape_frames(97, 131)
    a = _device(ctxs[route], fr[:, None])
    b = _device(ctxs[route], fr[:, None])
    assert a[0] == 0 and b[0] == 0 and a[1].tobytes() == b[1].tobytes()


def test_both_routes_same_bits(ctxs):
    fr = qc.shape_frames(193, 196)
    a, b = _device(ctxs[RESIDENT], fr[:, None]), _device(ctxs[TILED], fr[:, None])
    assert a[0] == 0 and b[0] == 0 and a[1].tobytes() == b[1].tobytes()


@pytest.mark.parametrize("route", ROUTES)
def test_host_entry(ctxs, route):
    H, W = 61, 75
    fr = np.stack([np.stack([qc.planet(H, W, 3 * f + c + 1, amp=300 * (c + 1) * (f + 1)) for c in range(3)]) for f in range(3)])
    before = fr.copy()
    rc, q = ctxs[route].quality(fr, layer=1)
    assert rc == 0, ctxs[route].error()
    _check(("host layer 1", route), q, want_of("layer1", fr[:, 1]))
    rc, q = ctxs[route].quality(fr, layer=1, included=[1, 0, 1], fill=SENTINEL)
    assert rc == 0 and q[1] == SENTINEL
    _check(("host holes", route), q[[0, 2]], want_of("layer1", fr[:, 1])[[0, 2]])
    assert np.array_equal(fr, before)
    rc, q = ctxs[route].quality(qc.shape_frames(6, 20))
    assert rc == 0 and (q == 0.0).all() and ctxs[route].quality_last_times()[1:] == (NONE, 0)


def register_ecc_literal(planes, ref_image, incl, process_all_frames, failed):
    """registration.c:833-921 with findTransform's outcome given: returns (quality, incl afterwards,
    q_min, q_max, q_index)"""
    n = len(planes)
    incl = list(incl)
    quality = [0.0] * n                                                  # calloc'ed regdata
    quality[ref_image] = orc.quality(planes[ref_image])                  # :833
    q_min = q_max = quality[ref_image]                                   # :838
    q_index = ref_image
    for frame in range(n):                                               # :853
        if not process_all_frames and not incl[frame]:
            continue
        if frame != ref_image:
            if failed[frame]:                                            # :878-890
                incl[frame] = 0
                continue
            quality[frame] = orc.quality(planes[frame])                  # :892
            qual = quality[frame]
            if qual > q_max:                                             # :900
                q_max = qual
                q_index = frame
            q_min = q_min if q_min < qual else qual                      # :904
    for frame in range(n):                                               # normalizeQualityData :163-176
        if not process_all_frames and not incl[frame]:
            continue
        v = np.float64(quality[frame]) - np.float64(q_min)
        with np.errstate(all="ignore"):
            quality[frame] = float(v / (np.float64(q_max) - np.float64(q_min)))
    return quality, incl, q_min, q_max, q_index


@pytest.mark.parametrize("process_all_frames", [False, True])
def test_register_ecc_glue(gpu_ctx, process_all_frames):
    """the whole glue of INTEGRATION.md on the 24 x 32 scene of tests/ecc_ref.py: ECC first (its failures
    exclude frames), one quality call with included & !failed, sg_quality_normalize, the best-frames filter"""
    import torch
    H, W = 24, 32
    a = er.scene(H, W, 1, [(0, 0), (1.3, -0.7), (4.7, -4.2), (-2.25, 1.8), (0.6, 2.1)])
    x100 = (a[0].astype(np.uint32) * 100).clip(0, 65535).astype(np.uint16)
    fr = np.stack([a[1], a[0], np.zeros_like(a[0]), x100, a[2], a[3], a[4]])
    n, ref_image = len(fr), 1
    seq_incl = np.array([1, 1, 1, 1, 1, 0, 1], dtype=np.int32)
    d = torch.from_numpy(fr.view(np.int16).copy()).cuda()
    torch.cuda.synchronize()
    todo = np.ones(n, dtype=np.int32) if process_all_frames else seq_incl
    rc, res = gpu_ctx.register_ecc_device(d.data_ptr(), n, H, W, ref_image=ref_image, included=todo)
    assert rc == 0, gpu_ctx.error()
    failed = (res["failed"] != 0) & (todo != 0)
    assert failed.tolist() == [False, False, True, True, True, False, False]
    measured = (todo != 0) & ~failed
    rc, raw = gpu_ctx.quality_device(d.data_ptr(), n, H, W, included=measured.astype(np.int32))
    assert rc == 0, gpu_ctx.error()
    incl_after = seq_incl & ~failed
    normalized = np.ones(n, dtype=bool) if process_all_frames else incl_after != 0
    q, q_min, q_max, q_index = sg.normalize_quality(raw, ref_image=ref_image, measured=measured, normalized=normalized)
    wq, wincl, wmin, wmax, widx = register_ecc_literal(fr, ref_image, seq_incl, process_all_frames, failed)
    print(f"ecc glue all={process_all_frames} q={q.tolist()} want={wq} min={q_min} max={q_max} index={q_index}")
    assert qc.same(q, wq) and (q_min, q_max, q_index) == (wmin, wmax, widx)
    assert incl_after.tolist() == wincl
    assert np.isfinite(q[measured]).all() and q[q_index] == 1.0 and q.min() <= 0.0
    # "stack the best 50 %": the literal lines of stacking.c on the same values
    thr, sel = sg.select_by_quality(q, 50.0, included=incl_after)
    val = sorted(q.tolist())
    wthr = val[int((100.0 - 50.0) * float(n) / 100.0)]
    assert thr == wthr and sel.tolist() == [i for i in range(n) if incl_after[i] and q[i] > 0.0 and q[i] >= wthr]
    assert len(sel) > 0


REFUSED = [dict(W=0), dict(H=0), dict(H=-4), dict(W=65536, H=32768), dict(N=0), dict(N=-2), dict(row_pitch=31),
           dict(frame_pitch=23 * 32 + 31), dict(row_pitch=40, frame_pitch=24 * 32)]


@pytest.mark.parametrize("i", range(len(REFUSED)))
def test_refusals_touch_nothing(gpu_ctx, i):
    import torch
    a = dict(N=2, H=24, W=32, row_pitch=0, frame_pitch=0)
    a.update(REFUSED[i])
    src = qc.shape_frames(24, 32).reshape(-1)
    d = torch.from_numpy(src.view(np.int16).copy()).cuda()
    torch.cuda.synchronize()
    q = np.full(4, SENTINEL)
    P = sg.ctypes.c_void_p
    rc = gpu_ctx.lib.sg_quality_u16_device(gpu_ctx.ctx, 0, P(d.data_ptr()), a["frame_pitch"], a["row_pitch"], a["W"], a["H"],
                                           a["N"], None, q.ctypes.data_as(P), None)
    torch.cuda.synchronize()
    assert rc == sg.SG_ERR_SIZE and gpu_ctx.error().startswith("quality:"), (rc, gpu_ctx.error())
    assert (q == SENTINEL).all() and np.array_equal(d.cpu().numpy().view(np.uint16), src)
    rc = gpu_ctx.lib.sg_quality_u16(gpu_ctx.ctx, P(src.ctypes.data), a["frame_pitch"], a["row_pitch"], a["W"], a["H"], a["N"],
                                    None, q.ctypes.data_as(P))
    assert rc == sg.SG_ERR_SIZE and gpu_ctx.error().startswith("quality:") and (q == SENTINEL).all()


def test_missing_pointers(gpu_ctx):
    q = np.full(2, SENTINEL)
    P = sg.ctypes.c_void_p
    rc = gpu_ctx.lib.sg_quality_u16_device(gpu_ctx.ctx, 0, None, 0, 0, 32, 24, 2, None, q.ctypes.data_as(P), None)
    assert rc == sg.SG_ERR_GENERIC and gpu_ctx.error().startswith("quality:") and (q == SENTINEL).all()
    with pytest.raises(ValueError, match="outside"):
        sg.select_by_quality([0.2, 0.4], 0.0)
    with pytest.raises(ValueError, match="NaN"):
        sg.select_by_quality([0.2, float("nan")], 50.0)
    with pytest.raises(ValueError, match="ref_image"):
        sg.normalize_quality([0.2, 0.4], ref_image=2)
