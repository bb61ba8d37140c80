"""Per-frame normalisation statistics: the device IKSS location / scale
(sg_frame_stats_ikss_device, sg_frame_stats_ikss) against the oracle's restatement of
statistics() (bit for bit), and compute_normalization through the C ABI against the oracle
(CPU).  The solver alone is fuzzed on the host by tests/test_ikss_cpu.py; the cases here are
about what only the device has: histogram chunks (SG_ST_CHUNK = 65535 samples per
workgroup, u16 LDS counters), the maximum over all layers, 64-frame solver blocks, 256-frame
passes and frame strides."""
import numpy as np
import pytest

import oracle_lib as orc
import sirilgpu as sg


@pytest.mark.parametrize("mode", [sg.ADDITIVE, sg.MULTIPLICATIVE, sg.ADDITIVE_SCALING, sg.MULTIPLICATIVE_SCALING])
def test_compute_normalization_matches_oracle(mode):
    rng = np.random.default_rng(mode)
    loc = 1000 + rng.random(9) * 50
    scl = 30 + rng.random(9) * 5
    for ref in (0, 4):
        want = orc.compute_normalization(mode, loc, scl, ref_image=ref)
        got = sg.compute_normalization(mode, loc, scl, ref_image=ref)
        for a, b in zip(got, want):
            assert np.array_equal(a, b)


def _frames():
    rng = np.random.default_rng(7)
    fr = []
    # synthetic star field with shifts / zeros / cosmics (sg_synth), 3 layers
    fr.append(orc.synth(1, 3, 96, 130, seed=5, maxshift=4)[0])
    fr.append(orc.synth(1, 3, 96, 130, seed=6, maxshift=4)[0])
    # 8-bit data (normalised by 255, utils.c:454-459), with zeros (null pixels)
    g = rng.normal(100, 12, size=(3, 96, 130)).clip(0, 255).astype(np.uint16)
    g[0, :5, :] = 0
    fr.append(g)
    # wide 16-bit distribution with outliers
    h = rng.normal(20000, 900, size=(3, 96, 130)).clip(0, 65535).astype(np.uint16)
    h[0, 10:12, :] = 65535
    fr.append(h)
    # nearly constant frame (mad == 0 / sigma == 0 exits)
    c = np.full((3, 96, 130), 777, dtype=np.uint16)
    c[0, 0, :7] = 778
    fr.append(c)
    return np.stack(fr)


@pytest.mark.gpu
def test_ikss_matches_oracle(gpu_ctx):
    import torch
    frames = _frames()
    N, C, H, W = frames.shape
    d = torch.from_numpy(frames.view(np.int16).reshape(-1).copy()).cuda()
    torch.cuda.synchronize()
    rc, loc, scl = gpu_ctx.frame_stats_ikss(d.data_ptr(), N, C, H, W)
    assert rc == 0, gpu_ctx.error()
    for i in range(N):
        orc_rc, l, s = orc.statistics_ikss(frames[i])
        assert orc_rc == 0
        assert loc[i] == l and scl[i] == s, (i, loc[i], l, scl[i], s)


@pytest.mark.gpu
def test_ikss_empty_frame_fails(gpu_ctx):
    import torch
    frames = np.zeros((2, 1, 16, 16), dtype=np.uint16)
    frames[1, 0, 3, 3] = 9
    d = torch.from_numpy(frames.view(np.int16).reshape(-1).copy()).cuda()
    torch.cuda.synchronize()
    rc, loc, scl = gpu_ctx.frame_stats_ikss(d.data_ptr(), 2, 1, 16, 16)
    assert rc != 0
    assert orc.statistics_ikss(frames[0])[0] != 0
    assert (loc[1], scl[1]) == orc.statistics_ikss(frames[1])[1:]


def _same(a, b):
    return np.float64(a).tobytes() == np.float64(b).tobytes()


def _device_stats(gpu_ctx, frames, gap=0):
    """(rc, location, scale) of frames [N][C][H][W] from a device buffer whose frames lie
    C*H*W + gap samples apart (the gaps hold 65535s, which no frame may see)"""
    import torch
    N, C, H, W = frames.shape
    stride = C * H * W + gap
    buf = np.full(N * stride, 65535, dtype=np.uint16)
    for i in range(N):
        buf[i * stride:i * stride + C * H * W] = frames[i].reshape(-1)
    d = torch.from_numpy(buf.view(np.int16)).cuda()
    torch.cuda.synchronize()
    return gpu_ctx.frame_stats_ikss(d.data_ptr(), N, C, H, W, frame_stride=stride if gap else 0)


def _check(gpu_ctx, frames, gap=0):
    """every frame's device result equals the oracle's; returns the oracle's [(location, scale)]"""
    rc, loc, scl = _device_stats(gpu_ctx, frames, gap)
    assert rc == 0, gpu_ctx.error()
    want = []
    for i in range(frames.shape[0]):
        orc_rc, l, s = orc.statistics_ikss(frames[i])
        assert orc_rc == 0
        assert _same(loc[i], l) and _same(scl[i], s), (i, loc[i], l, scl[i], s)
        want.append((l, s))
    return want


def _gauss(seed, mean, sigma, shape):
    return np.random.default_rng(seed).normal(mean, sigma, size=shape).clip(0, 65535).astype(np.uint16)


@pytest.mark.gpu
@pytest.mark.parametrize("H,W", [(255, 257), (256, 256), (300, 437)])
def test_ikss_chunk_edges(gpu_ctx, H, W):
    """exactly one histogram chunk (65535 pixels), a second chunk of one pixel, and
    2 * 65535 + 30 pixels: the global histogram and the maximum are merged across workgroups"""
    assert (H * W) % 65535 in (0, 1, 30)
    _check(gpu_ctx, _gauss(H, 20000, 900, (1, 1, H, W)))


@pytest.mark.gpu
def test_ikss_counter_saturation(gpu_ctx):
    """one value nearly fills a chunk: a u16 LDS counter (low half for an even value, high half
    for an odd one) reaches 65533 / 65535 and must neither wrap nor carry into its pair"""
    even = np.full(256 * 256, 776, dtype=np.uint16)
    even[[7, 30000, 65535]] = 777        # 65533 x 776 and 2 x 777 in chunk 0, one 777 in chunk 1
    odd = np.where(even == 776, 777, 776).astype(np.uint16)
    want = _check(gpu_ctx, np.stack([even, odd]).reshape(2, 1, 256, 256))
    assert want[0] == (776.0, 0.0) and want[1] == (777.0, 0.0)
    full = np.full((1, 1, 255, 257), 776, dtype=np.uint16)      # the low counter at exactly 65535
    assert _check(gpu_ctx, full) == [(776.0, 0.0)]
    two = np.full(300 * 437, 1001, dtype=np.uint16)     # chunk 1: 65535 x 1001 in a high half
    two[:40000] = 1000
    assert _check(gpu_ctx, two.reshape(1, 1, 300, 437)) == [(1001.0, 0.0)]


@pytest.mark.gpu
def test_ikss_norm_decided_by_another_layer(gpu_ctx):
    """norm (255 or 65535) follows the maximum over all layers: one pixel of 300 in layer 2,
    in the second chunk, changes the statistics of layer 0"""
    a = np.random.default_rng(21).integers(1, 256, size=(1, 3, 260, 260)).astype(np.uint16)
    b = a.copy()
    b[0, 2, -1, -1] = 300
    assert 260 * 260 - 1 >= 65535
    ra, rb = orc.statistics_ikss(a[0]), orc.statistics_ikss(b[0])
    assert ra[0] == 0 and rb[0] == 0 and ra != rb, (ra, rb)     # else the case proves nothing
    assert _check(gpu_ctx, a) == [ra[1:]]
    assert _check(gpu_ctx, b) == [rb[1:]]


@pytest.mark.gpu
def test_ikss_many_frames_strided(gpu_ctx):
    """257 frames: five 64-lane solver blocks, a second host pass (f0 = 256) of one frame, and a
    frame stride of C*H*W + 7; then the last frame empty"""
    N, H, W = 257, 24, 40
    rng = np.random.default_rng(33)
    frames = np.stack([rng.normal(500 + 100 * i, 5 + i, size=(1, H, W)).clip(0, 65535).astype(np.uint16)
                       for i in range(N)])
    want = _check(gpu_ctx, frames, gap=7)
    frames[256] = 0
    rc, loc, scl = _device_stats(gpu_ctx, frames, gap=7)
    assert rc != 0
    assert orc.statistics_ikss(frames[256])[0] != 0
    for i in range(256):
        assert _same(loc[i], want[i][0]) and _same(scl[i], want[i][1]), i


@pytest.mark.gpu
def test_ikss_extremes(gpu_ctx):
    rng = np.random.default_rng(44)
    two_values = np.where(rng.random((16, 16)) < 0.5, 1, 65535).astype(np.uint16)
    top = np.full((16, 16), 65535, dtype=np.uint16)
    one = np.zeros((16, 16), dtype=np.uint16)
    one[5, 9] = 65535
    two = np.zeros((16, 16), dtype=np.uint16)
    two[0, 0], two[15, 15] = 12345, 54321
    _check(gpu_ctx, np.stack([two_values, top, one, two]).reshape(4, 1, 16, 16))


@pytest.mark.gpu
def test_ikss_clipping(gpu_ctx):
    """10 % uniform outliers around a tight gaussian: the 4-sigma clipping moves both ends"""
    rng = np.random.default_rng(55)
    f = rng.normal(2000, 30, size=300 * 437).clip(0, 65535).astype(np.uint16)
    out = rng.random(f.size) < 0.1
    f[out] = rng.integers(0, 65536, size=int(out.sum())).astype(np.uint16)
    _check(gpu_ctx, f.reshape(1, 1, 300, 437))


@pytest.mark.gpu
def test_ikss_host_entry(gpu_ctx):
    """sg_frame_stats_ikss: an empty frame in the middle is reported, the others are computed"""
    frames = np.stack([_gauss(61, 3000, 40, (3, 50, 70)), np.zeros((3, 50, 70), dtype=np.uint16),
                       _gauss(62, 150, 20, (3, 50, 70)).clip(0, 255)])
    rc, loc, scl = gpu_ctx.frame_stats_ikss_host(frames)
    assert rc == sg.SG_ERR_GENERIC
    assert orc.statistics_ikss(frames[1])[0] != 0
    for i in (0, 2):
        orc_rc, l, s = orc.statistics_ikss(frames[i])
        assert orc_rc == 0
        assert _same(loc[i], l) and _same(scl[i], s), (i, loc[i], l, scl[i], s)
