"""Sequence preprocessing on the device (sg_prepro_*) against tests/prepro_ref.py,
bit for bit: the fused calibration (every subset of the masters, vector body / scalar tail / frame
gaps), the background noise of dark-subtracted frames (the dark fit's objective, every row shape
the compaction and the clip passes can meet), the dark fit end to end, the cosmetic correction
through the component schedule, the refused regimes, the host entry and the hand-off of calibrated
frames to the stack without leaving HBM."""
import numpy as np
import pytest

import oracle_lib as orc
import prepro_ref as pr
import sirilgpu as sg

pytestmark = pytest.mark.gpu

GAP_FILL = 0xABCD


def _run(ctx, pp, frames, gap=0, want_k=True):
    """calibrate frames [N][C][H][W] in place on the device, C*H*W + gap samples apart; the gaps
    (and a guard after the last frame) must come back untouched: (rc, frames, k)"""
    import torch
    N = frames.shape[0]
    total = frames[0].size
    stride = total + gap
    buf = np.full(N * stride + 64, GAP_FILL, dtype=np.uint16)
    for i in range(N):
        buf[i * stride:i * stride + total] = frames[i].reshape(-1)
    d = torch.from_numpy(buf.view(np.int16)).cuda()
    torch.cuda.synchronize()
    rc, k = ctx.prepro_frames_device(pp, d.data_ptr(), N, frame_stride=stride if gap else 0, want_k=want_k)
    torch.cuda.synchronize()
    got = d.cpu().numpy().view(np.uint16)
    out = np.stack([got[i * stride:i * stride + total].reshape(frames.shape[1:]) for i in range(N)])
    for i in range(N):
        assert (got[i * stride + total:(i + 1) * stride] == GAP_FILL).all(), f"gap after frame {i} written"
    assert (got[N * stride:] == GAP_FILL).all(), "guard written"
    return rc, out, k


def _noise(ctx, pp, frames, ks):
    import torch
    d = torch.from_numpy(np.ascontiguousarray(frames).view(np.int16).reshape(-1).copy()).cuda()
    torch.cuda.synchronize()
    rc, noise = ctx.prepro_noise_device(pp, d.data_ptr(), frames.shape[0], ks)
    assert rc == 0, ctx.error()
    assert np.array_equal(d.cpu().numpy().view(np.uint16), frames.reshape(-1)), "the frames changed"
    return noise


def _same(a, b):
    return np.float64(a).tobytes() == np.float64(b).tobytes()


# ------------------------------------------------------------------ calibration

def _masters(rng, C, H, W):
    off = rng.integers(0, 2000, size=(C, H, W)).astype(np.uint16)
    dark = rng.integers(0, 3000, size=(C, H, W)).astype(np.uint16)
    dark[rng.random((C, H, W)) < 0.05] = 65535
    flat = rng.integers(1, 60000, size=(C, H, W)).astype(np.uint16)
    flat[rng.random((C, H, W)) < 0.1] = 0
    flat[rng.random((C, H, W)) < 0.1] = 3          # small divisors: the quotient passes 65535
    return off, dark, flat


@pytest.mark.parametrize("C", [1, 3])
@pytest.mark.parametrize("H,W", [(1, 1), (2, 3), (5, 63), (4, 64), (3, 65), (9, 257), (3, 1031)])
def test_calibration_every_subset(gpu_ctx, H, W, C):
    rng = np.random.default_rng(1000 * C + W)
    off, dark, flat = _masters(rng, C, H, W)
    for subset in range(8):
        use = dict(offset=off if subset & 1 else None, dark=dark if subset & 2 else None, flat=flat if subset & 4 else None)
        N, gap = [(1, 0), (2, 5), (7, 8), (2, 0), (7, 3), (1, 8), (2, 16), (7, 0)][subset]
        autolevel = bool(subset & 4) and bool((subset + C) & 1) and pr.auto_level(flat) is not None
        norm = 1234.5678
        frames = rng.integers(0, 65536, size=(N, C, H, W)).astype(np.uint16)
        frames[rng.random(frames.shape) < 0.05] = 0
        with sg.Prepro(gpu_ctx, W, H, C, autolevel=autolevel, normalisation=norm, **use) as pp:
            info = pp.info()
            rc, got, k = _run(gpu_ctx, pp, frames, gap)
        assert rc == 0, gpu_ctx.error()
        want, _ = pr.preprocess(frames, autolevel=autolevel, normalisation=norm, **use)
        assert np.array_equal(got, want), (subset, N, gap, np.argwhere(got != want)[:5])
        assert (k == 1.0).all() and info.cosmetic_applies == 0
        if use["flat"] is not None:
            assert info.level == (pr.auto_level(flat) if autolevel else float(np.float32(norm)))
            assert W < 63 or ((want == 65535).any() and (want == 0).any())      # saturates both ways


def test_calibration_flat_half_rounding(gpu_ctx):
    """level * (v / f) landing exactly on x.5 rounds up; the level is a float"""
    raw = np.array([[[[3, 1, 60000, 0, 5, 5, 5, 5, 5]]]], dtype=np.uint16)
    flat = np.array([[[2, 1, 1, 0, 1, 2, 4, 10, 0]]], dtype=np.uint16)
    for level in (1.5, 2.5, 0.1):
        with sg.Prepro(gpu_ctx, 9, 1, 1, flat=flat, normalisation=level) as pp:
            rc, got, _ = _run(gpu_ctx, pp, raw)
        assert rc == 0 and np.array_equal(got[0], pr.calibrate(raw[0], flat=flat, level=level))
    assert pr.calibrate(raw[0], flat=flat, level=2.5)[0, 0, :3].tolist() == [4, 3, 65535]
    assert pr.calibrate(raw[0], flat=flat, level=0.1)[0, 0, 4] == 1     # 5 * 0.1f = 0.50000000745 -> 1


# ------------------------------------------------------------------ noise

KS = [0.0, 0.37, 1.0, 2.0]


def _noise_frame(rng, H, W):
    """a frame and a dark whose rows cover the compaction's cases as far as H and W allow"""
    raw = rng.normal(1200, 25, size=(H, W)).clip(1, 65535).astype(np.uint16)
    raw[rng.random((H, W)) < 0.15] = 0
    dark = rng.integers(0, 60, size=(H, W)).astype(np.uint16)
    if H >= 8:
        raw[0] = 0                                              # all zero
        for y, nz in ((1, 1), (2, 2), (3, 3)):                  # exactly 1, 2, 3 non-zero pixels
            raw[y] = 0
            raw[y, rng.choice(W, min(nz, W), replace=False)] = 40000
        raw[4, :min(5, W)] = 0                                  # zeros at the start, the end and across pixel 63 | 64
        raw[4, -min(7, W):] = 0
        raw[4, 60:70] = 0
        raw[4, 250:262] = 0                                     # ... and across a 256-pixel step
        if W > 256:
            raw[6, 255], raw[7, 256] = 0, 0
            raw[6, 252:255], raw[7, 257:260] = 901, 902
        raw[5] = 777                                            # constant: stdev 0
        dark[5] = 0
    return raw, dark


@pytest.mark.parametrize("W,H", [(2, 3), (3, 1), (4, 2), (63, 3), (64, 8), (65, 8), (129, 8), (1025, 8), (4099, 3),
                                 (65535, 2)])
def test_noise_matches_reference(gpu_ctx, W, H):
    rng = np.random.default_rng(W)
    raw, dark = _noise_frame(rng, H, W)
    frames = np.stack([raw] * len(KS))[:, None]
    for k in KS:
        assert not pr.has_nan_row(raw, dark, k)
    with sg.Prepro(gpu_ctx, W, H, 1, dark=dark) as pp:
        got = _noise(gpu_ctx, pp, frames, KS)
    for i, k in enumerate(KS):
        want = pr.objective(raw, dark, k)
        assert _same(got[i], want), (W, H, k, got[i], want)
    if W == 2:
        assert (got == 0.0).all()


def test_noise_clip_passes(gpu_ctx):
    """rows built so that 0, 1, 2 and 3 clip passes run (the third still dropping something), one
    row per frame so that each row's value is the image's"""
    rows = pr.edge_rows()
    W = max(len(r) for _, r, _ in rows)
    frames = np.zeros((len(rows), 1, 1, W), dtype=np.uint16)
    for i, (_, r, _) in enumerate(rows):
        frames[i, 0, 0, :len(r)] = r
    dark = np.zeros((1, W), dtype=np.uint16)
    seen, third = set(), False
    with sg.Prepro(gpu_ctx, W, 1, 1, dark=dark) as pp:
        got = _noise(gpu_ctx, pp, frames, np.full(len(rows), 1.0))
    for i, (name, r, _) in enumerate(rows):
        ran, dropped = [], []
        s = pr.noise_row_rule(frames[i, 0, 0], ran, dropped)
        seen.update(ran)
        third = third or (len(dropped) == 3 and dropped[2] > 0)
        want = .70710678 * (s if s is not None else 0.0)
        assert _same(got[i], want), (name, got[i], want)
    assert seen >= {0, 1, 2, 3} and third


def test_noise_frame_emptied_by_k(gpu_ctx):
    """k = 2 leaves no non-zero pixel: statistics() is NULL, the objective 0.0; many frames and
    different k in one call"""
    rng = np.random.default_rng(77)
    dark = rng.integers(500, 900, size=(6, 90)).astype(np.uint16)
    raw = (dark.astype(np.int64) * 2 - rng.integers(0, 40, size=dark.shape)).astype(np.uint16)
    N = 300                                     # more than one batch of 256 evaluations
    ks = np.linspace(0.0, 2.0, N)
    frames = np.stack([raw] * N)[:, None]
    assert pr.objective(raw, dark, 2.0) == 0.0 and pr.objective(raw, dark, 1.9) > 0.0
    with sg.Prepro(gpu_ctx, 90, 6, 1, dark=dark) as pp:
        got = _noise(gpu_ctx, pp, frames, ks)
    for i in (0, 1, 100, 255, 256, 284, 299):
        assert not pr.has_nan_row(raw, dark, ks[i])
        assert _same(got[i], pr.objective(raw, dark, ks[i])), i
    assert got[-1] == 0.0


# ------------------------------------------------------------------ dark fit

K_TRUE = [0.6, 1.0, 1.4]
_fit_cache = {}


def _fit(H, W):
    """(frames, dark, reference k per frame), computed once per shape"""
    if (H, W) not in _fit_cache:
        frames, dark = pr.fit_case(H, W, K_TRUE, seed=H + W)
        ks = [pr.search_rule(lambda k: pr.objective(frames[i, 0], dark, k)) for i in range(len(K_TRUE))]
        assert all(it == 13 for _, it in ks)
        _fit_cache[(H, W)] = (frames, dark, np.array([k for k, _ in ks]))
    return _fit_cache[(H, W)]


@pytest.mark.parametrize("H,W", [(9, 67), (33, 130), (64, 257)])
def test_dark_fit_end_to_end(gpu_ctx, H, W):
    frames, dark, k_ref = _fit(H, W)
    rng = np.random.default_rng(H)
    off = rng.integers(90, 110, size=(1, H, W)).astype(np.uint16)
    flat = rng.normal(30000, 2000, size=(1, H, W)).clip(1, 65535).astype(np.uint16)
    flat[0, 0, :3] = 0
    for use_off in (False, True):
        for use_flat in (False, True):
            kw = dict(offset=off if use_off else None, flat=flat if use_flat else None, autolevel=use_flat)
            with sg.Prepro(gpu_ctx, W, H, 1, dark=dark[None], dark_optimization=True, **kw) as pp:
                rc, got, k = _run(gpu_ctx, pp, frames, gap=8 if use_off else 0)
            assert rc == 0, gpu_ctx.error()
            assert k.tobytes() == k_ref.tobytes(), (k, k_ref)                       # 1. the fitted k, bitwise
            level = pr.auto_level(flat) if use_flat else 1.0
            for i in range(len(K_TRUE)):                                            # 2. each calibrated frame
                want = pr.calibrate(frames[i], kw["offset"], dark[None], kw["flat"], level, optd_k=k_ref[i])
                assert np.array_equal(got[i], want), (use_off, use_flat, i)
    assert (np.abs(k_ref - np.array(K_TRUE)) < 0.05).all(), k_ref                   # 3. sanity only


def test_dark_fit_null_k_and_single_frame(gpu_ctx):
    frames, dark, k_ref = _fit(9, 67)
    with sg.Prepro(gpu_ctx, 67, 9, 1, dark=dark[None], dark_optimization=True) as pp:
        rc, got, k = _run(gpu_ctx, pp, frames[1:2], want_k=False)
    assert rc == 0 and k is None
    assert np.array_equal(got[0], pr.calibrate(frames[1], dark=dark[None], optd_k=k_ref[1]))


# ------------------------------------------------------------------ cosmetic correction

def _cosmetic_case(gpu_ctx, dark, sig, cfa, N=3, C=1, seed=0):
    H, W = dark.shape[-2:]
    rng = np.random.default_rng(seed)
    frames = rng.normal(3000, 400, size=(N, C, H, W)).clip(0, 65535).astype(np.uint16)
    frames[0] = rng.integers(0, 65536, size=(C, H, W))
    with sg.Prepro(gpu_ctx, W, H, C, dark=dark, cosmetic=True, cosme_sigma=sig, is_cfa=cfa) as pp:
        info = pp.info()
        rc, got, _ = _run(gpu_ctx, pp, frames, gap=5)
    assert rc == 0, gpu_ctx.error()
    want, _ = pr.preprocess(frames, dark=dark, cosmetic=True, cosme_sigma=sig, is_cfa=cfa)
    assert np.array_equal(got, want), np.argwhere(got != want)[:8]
    return info, frames, want


@pytest.mark.parametrize("cfa", [False, True])
@pytest.mark.parametrize("H,W", [(9, 7), (64, 64), (70, 130)])
def test_cosmetic_clusters(gpu_ctx, H, W, cfa):
    dark = pr.cluster_dark(H, W, seed=H)
    info, frames, want = _cosmetic_case(gpu_ctx, dark[None], pr.CLUSTER_SIG, cfa, seed=W)
    dev = pr.find_deviant(dark, pr.CLUSTER_SIG)
    comps = pr.components(dev, W, H, cfa)
    assert info.cosmetic_applies == 1 and info.ihot >= H + W - 1 and info.icold > 0
    assert info.ihot + info.icold == len(dev)
    assert info.components == len(comps) and info.longest_component == max(len(c) for c in comps)
    t = pr.thresholds(dark, pr.CLUSTER_SIG)
    assert (info.dark_sigma, info.dark_median, info.thres_cold, info.thres_hot) == t
    # the correction changed something beyond the dark subtraction
    assert not np.array_equal(want, pr.preprocess(frames, dark=dark[None])[0])


@pytest.mark.parametrize("cfa", [False, True])
def test_cosmetic_every_pixel_deviant(gpu_ctx, cfa):
    dark = pr.cluster_dark(12, 16, seed=2, every=True)
    info, _, _ = _cosmetic_case(gpu_ctx, dark[None], (0.5, 0.5), cfa)
    assert info.ihot + info.icold == 12 * 16 and info.components == (4 if cfa else 1)


def test_cosmetic_flags_skips_and_empty_list(gpu_ctx):
    dark = pr.cluster_dark(20, 24, seed=3)
    cold_off, _, _ = _cosmetic_case(gpu_ctx, dark[None], (-1.0, pr.CLUSTER_SIG[1]), False)
    hot_off, _, _ = _cosmetic_case(gpu_ctx, dark[None], (pr.CLUSTER_SIG[0], -1.0), False)
    assert cold_off.icold == 0 and cold_off.ihot > 0 and cold_off.thres_cold == -1.0
    assert hot_off.ihot == 0 and hot_off.icold > 0 and hot_off.thres_hot == 65536.0
    none, _, _ = _cosmetic_case(gpu_ctx, dark[None], (-1.0, -1.0), False)           # empty list
    assert none.cosmetic_applies == 1 and none.ihot + none.icold == 0 and none.components == 0
    dark3 = np.stack([dark, dark, dark])                                            # 3 layers: skipped, and said so
    info, _, _ = _cosmetic_case(gpu_ctx, dark3, pr.CLUSTER_SIG, False, C=3)
    assert info.cosmetic_applies == 0 and info.ihot + info.icold == 0


# ------------------------------------------------------------------ refusals, host entry, hand-off

def test_refused_regimes(gpu_ctx):
    m1, m3 = np.ones((1, 4, 4), dtype=np.uint16), np.ones((3, 4, 4), dtype=np.uint16)
    cases = [(dict(nb_layers=3, dark=m3, dark_optimization=True), sg.SG_ERR_GENERIC, "nb_layers != 1"),
             (dict(nb_layers=1, dark_optimization=True), sg.SG_ERR_GENERIC, "dark optimization needs a master dark"),
             (dict(nb_layers=1, cosmetic=True), sg.SG_ERR_GENERIC, "cosmetic correction needs a master dark"),
             (dict(nb_layers=1, flat=np.zeros((1, 4, 4), dtype=np.uint16), autolevel=True), sg.SG_ERR_GENERIC,
              "no non-zero pixel")]
    for kw, code, text in cases:
        with pytest.raises(RuntimeError, match=f"\\({code}\\)"):
            sg.Prepro(gpu_ctx, 4, 4, **kw)
        assert text in gpu_ctx.error(), gpu_ctx.error()
    d = sg.PreproDesc()
    for w, h, c in ((0, 4, 1), (4, -2, 1), (4, 4, 0)):
        d.width, d.height, d.nb_layers = w, h, c
        import ctypes
        hnd = ctypes.c_void_p()
        assert gpu_ctx.lib.sg_prepro_create(gpu_ctx.ctx, 0, ctypes.byref(d), ctypes.byref(hnd)) == sg.SG_ERR_SIZE
        assert not hnd.value
    # the objective without a dark
    import torch
    t = torch.zeros(16, dtype=torch.int16, device="cuda")
    with sg.Prepro(gpu_ctx, 4, 4, 1, offset=m1) as pp:
        rc, _ = gpu_ctx.prepro_noise_device(pp, t.data_ptr(), 1, [1.0])
    assert rc == sg.SG_ERR_GENERIC and "needs a master dark" in gpu_ctx.error()


def test_host_entry_equals_device_entry(gpu_ctx):
    frames, dark, k_ref = _fit(9, 67)
    rng = np.random.default_rng(5)
    off = rng.integers(90, 110, size=(1, 9, 67)).astype(np.uint16)
    hot = dark.copy()
    with sg.Prepro(gpu_ctx, 67, 9, 1, offset=off, dark=hot[None], dark_optimization=True, cosmetic=True,
                   cosme_sigma=(3.0, 3.0)) as pp:
        assert pp.info().ihot > 0
        rc, dev_out, k_dev = _run(gpu_ctx, pp, frames)
        host = frames.copy()
        rc2, k_host = gpu_ctx.prepro_frames_host(pp, host)
    assert rc == 0 and rc2 == 0, gpu_ctx.error()
    assert np.array_equal(host, dev_out) and k_host.tobytes() == k_dev.tobytes() == k_ref.tobytes()
    want, _ = pr.preprocess(frames, offset=off, dark=hot[None], dark_optimization=True, cosmetic=True, cosme_sigma=(3.0, 3.0))
    assert np.array_equal(host, want)


def test_handoff_to_the_stack(gpu_ctx):
    """frames calibrated in place, then stacked (SUM and SIGMA) without leaving HBM"""
    import torch
    N, C, H, W = 12, 1, 40, 70
    frames = orc.synth(N, C, H, W, seed=21, maxshift=0)
    rng = np.random.default_rng(21)
    off = rng.integers(90, 110, size=(C, H, W)).astype(np.uint16)
    dark = rng.integers(0, 60, size=(C, H, W)).astype(np.uint16)
    dark[0, 7, 9] = dark[0, 20, :] = 50000
    flat = rng.normal(30000, 2000, size=(C, H, W)).clip(1, 65535).astype(np.uint16)
    kw = dict(offset=off, dark=dark, flat=flat, autolevel=True, cosmetic=True, cosme_sigma=(-1.0, 3.0))
    want, _ = pr.preprocess(frames, **kw)
    assert not np.array_equal(want, frames)
    d = torch.from_numpy(frames.view(np.int16).reshape(-1).copy()).cuda()
    o = torch.zeros(C * H * W, dtype=torch.int16, device="cuda")
    torch.cuda.synchronize()
    with sg.Prepro(gpu_ctx, W, H, C, **kw) as pp:
        assert pp.info().ihot >= W + 1
        rc, _ = gpu_ctx.prepro_frames_device(pp, d.data_ptr(), N)
    assert rc == 0, gpu_ctx.error()
    rc, ref_sum, _ = orc.stack_sum(want)
    assert rc == 0
    desc, keep = sg.make_desc(sg.SUM, N, W, H, C, max_thread=4, max_number_of_rows=H)
    gpu_ctx.stack_device(desc, d.data_ptr(), C * H * W, H * W, o.data_ptr(), 0, H)
    assert np.array_equal(o.cpu().numpy().view(np.uint16).reshape(C, H, W), ref_sum)
    rc, ref_sig, rej_ref = orc.stack_rejection(want, sg.SIGMA, sig=(3.0, 3.0), max_thread=4)
    assert rc == 0
    desc, keep = sg.make_desc(sg.MEAN, N, W, H, C, rejection=sg.SIGMA, sig=(3.0, 3.0), max_thread=4, max_number_of_rows=H)
    rej, _ = gpu_ctx.stack_device(desc, d.data_ptr(), C * H * W, H * W, o.data_ptr(), 0, H)
    assert np.array_equal(o.cpu().numpy().view(np.uint16).reshape(C, H, W), ref_sig)
    assert np.array_equal(rej, rej_ref)
