"""The resident-frame entry points past one batch of frames, one 64-candidate step and one sweep of a
capped grid: sg_findstar_device and sg_findstar_fit_device on 257 and 258 frames (chunks of 256),
sg_prepro_frames_device on 129 and 257 frames (chunks of 128) and their host entries, a frame that
stores 161 candidates with max_stars on both sides of the step boundaries, and frames large enough
that k_prepro_calibrate (4096 blocks) and k_findstar_copy (1024 blocks) sweep their grid twice.
Everything is compared as the single-batch tests compare it (their helpers are imported): bit for bit
with tests/findstar_ref.py and tests/prepro_ref.py, the fitted fields within psf_ref.TOL on stable
boxes.  tests/test_batches_cpu.py holds the conditions relied on here: the chunk sizes, the candidate
counts of the dense frame, the different k of the chunks' first frames and the sample counts against
the grid caps."""
import numpy as np
import pytest

import findstar_ref as fr
import prepro_ref as ppr
import psf_ref as pr
import sirilgpu as sg
import test_gpu_starfit as gs
from test_gpu_findstar import _check_record, _run as _find
from test_gpu_prepro import _masters, _run as _prepro
from test_gpu_starfit import _call, _check_frame

pytestmark = pytest.mark.gpu

K = pr.K_SIGMA


def _same_call(a, b):
    """two results of _call or _find are the same bytes"""
    assert a[0] == 0 and b[0] == 0
    assert [bytes(q) for q in a[1]] == [bytes(q) for q in b[1]]
    for x, y in zip(a[2:], b[2:]):
        assert (x is None) == (y is None) and (x is None or x.tobytes() == y.tobytes())


# ------------------------------------------------------------------ star candidates, 257 and 258 frames

_find_refs = {}


def _find_ref(plane, r, k, area):
    """(candidates, threshold record, detection plane, boxes), computed once per distinct plane"""
    key = (plane.tobytes(), r, k, area)
    if key not in _find_refs:
        cands, want, wave = fr.candidates(plane, k, r, area)
        _find_refs[key] = (cands, want, wave, fr.boxes(plane, cands, r))
    return _find_refs[key]


def _check_find(frames, got, r, k, maxc, area=None, records_only=False):
    rc, rec, xy, bx, wave = got
    assert rc == 0
    for f in range(frames.shape[0]):
        cands, want, wref, bref = _find_ref(frames[f, 0], r, k, area)
        _check_record(rec[f], want, len(cands), maxc)
        assert rec[f].wavelet_applied == 1 and rec[f].ratio_applied == 0 and rec[f].sigma_on_host == 0
        n = min(len(cands), maxc)
        assert (xy[f, n:] == 0).all() and (bx[f, n:] == 0).all()
        if records_only:
            assert n == 0
            continue
        assert np.array_equal(wave[f], wref), (f, np.argwhere(wave[f] != wref)[:5])
        assert xy[f, :n].tolist() == [list(c) for c in cands[:n]], (f, xy[f, :n].tolist(), cands[:n])
        assert np.array_equal(bx[f, :n], bref[:n]), f


def test_findstar_258_frames_second_chunk_of_an_empty_and_an_ordinary_frame(gpu_ctx):
    frames, which, _ = fr.batch_sequence(258, [-1, 3])
    kw = dict(maxc=10, gap=37)
    one = _find(gpu_ctx, frames[:1], 3, 1.0, **kw)
    got = _find(gpu_ctx, frames, 3, 1.0, **kw)
    assert got[0] == 0, gpu_ctx.error()
    _check_find(frames, got, 3, 1.0, 10)
    assert got[1][256].no_data == 1 and got[1][256].ncand == 0 and got[1][257].nstored >= 1
    assert got[2][257].tolist() != got[2][0].tolist()
    # without the caller's plane array the scratch plane of the chunk serves: the same answer
    _same_call(got[:4], _find(gpu_ctx, frames, 3, 1.0, want_wave=False, **kw)[:4])
    again = _find(gpu_ctx, frames[:1], 3, 1.0, **kw)
    _same_call(one, again)


def test_findstar_257_frames_lone_empty_frame_and_host_entry(gpu_ctx):
    """the second chunk stores nothing (total == 0); sg_findstar on the same frames returns the same bytes"""
    frames, _, _ = fr.batch_sequence(257, [-1])
    one = _find(gpu_ctx, frames[255:256], 3, 1.0, maxc=10)
    got = _find(gpu_ctx, frames, 3, 1.0, maxc=10, gap=37)
    assert got[0] == 0, gpu_ctx.error()
    _check_find(frames, got, 3, 1.0, 10)
    assert got[1][256].no_data == 1 and got[1][255].nstored >= 1
    nowave = _find(gpu_ctx, frames, 3, 1.0, maxc=10, gap=37, want_wave=False)
    _same_call(got[:4], nowave[:4])
    rc, rec, xy, bx, wave = gpu_ctx.findstar(frames, 3, 1.0, max_candidates=10, want_wave=True)
    assert rc == 0, gpu_ctx.error()
    _same_call(got, (rc, rec, xy, bx, wave))
    _same_call(one, _find(gpu_ctx, frames[255:256], 3, 1.0, maxc=10))


def test_findstar_257_frames_nothing_to_scan(gpu_ctx):
    """2r >= the area's width (scan_w == 0): every chunk ends after its records"""
    frames, _, _ = fr.batch_sequence(257, [3])
    area = fr.BATCH_EMPTY_AREA
    one = _find(gpu_ctx, frames[:1], 3, 1.0, area=area, maxc=10)
    got = _find(gpu_ctx, frames, 3, 1.0, area=area, maxc=10, gap=37)
    assert got[0] == 0, gpu_ctx.error()
    _check_find(frames, got, 3, 1.0, 10, area=area, records_only=True)
    assert bytes(got[1][256]) != bytes(got[1][0]) and got[1][256].ngood > 0
    _same_call(one, _find(gpu_ctx, frames[:1], 3, 1.0, area=area, maxc=10))


# ------------------------------------------------------------------ PSF fit, 257 and 258 frames

def _check_fit_frames(frames, which, planes, got, full, max_stars):
    rc, rec, nstars, st, cd = got
    first = {}
    for f, w in enumerate(which):
        if f in full:
            _check_frame(planes[w], rec[f], nstars[f], st[f], cd[f], 5, max_stars=max_stars)
        g = first.setdefault(w, f)
        assert bytes(rec[f]) == bytes(rec[g]) and nstars[f] == nstars[g], (f, g)
        assert st[f].tobytes() == st[g].tobytes() and cd[f].tobytes() == cd[g].tobytes(), (f, g)
        if w == 2:
            assert rec[f].no_data == 1 and rec[f].nstored == 0 and nstars[f] == 0
        else:       # as test_max_stars_keeps_the_first_in_raster_order requires of one frame
            assert nstars[f] == max_stars and (cd[f]["status"][:rec[f].nstored] == sg.SG_FIT_OVER_CAP).sum() >= 10


def test_starfit_258_frames(gpu_ctx):
    frames, which, planes = pr.starfit_batch_sequence(258)
    assert which[255:] == [0, 2, 1]
    kw = dict(maxc=64, max_stars=7, want_cands=True, gap=37)
    one = _call(gpu_ctx, frames[:1], 5, **kw)
    got = _call(gpu_ctx, frames, 5, **kw)
    assert got[0] == 0, gpu_ctx.error()
    _check_fit_frames(frames, which, planes, got, (0, 1, 2, 255, 256, 257), 7)
    _same_call(one, _call(gpu_ctx, frames[:1], 5, **kw))


def test_starfit_257_frames_lone_empty_frame_and_host_entry(gpu_ctx):
    frames, which, planes = pr.starfit_batch_sequence(257)
    kw = dict(maxc=64, max_stars=7, want_cands=True)
    one = _call(gpu_ctx, frames[1:2], 5, **kw)
    got = _call(gpu_ctx, frames, 5, **kw)
    assert got[0] == 0, gpu_ctx.error()
    _check_fit_frames(frames, which, planes, got, (0, 1, 2, 255, 256), 7)
    host = _call(gpu_ctx, frames, 5, host=True, **kw)
    assert host[0] == 0, gpu_ctx.error()
    _same_call(got, host)
    _same_call(one, _call(gpu_ctx, frames[1:2], 5, **kw))


# ------------------------------------------------------------------ calibration, 129 and 257 frames

_batch_fit = {}


def _batch_fit_case():
    """(frames, dark, offset, settings, reference frames, reference k), computed once"""
    if not _batch_fit:
        frames, dark, _ = ppr.batch_fit_case()
        off = np.random.default_rng(5).integers(90, 110, size=(1,) + ppr.BATCH_SHAPE).astype(np.uint16)
        kw = dict(offset=off, dark=dark[None], dark_optimization=True, cosmetic=True, cosme_sigma=(3.0, 3.0))
        want, ks = ppr.preprocess(frames, **kw)
        _batch_fit["case"] = (frames, kw, want, ks)
    return _batch_fit["case"]


@pytest.mark.parametrize("gap", [0, 5])
def test_prepro_257_frames_dark_fit_and_cosmetic(gpu_ctx, gap):
    """three chunks: the k of every frame, its own scaled dark and the cosmetic schedule per chunk; with
    gap 0 the host entry too, which works in batches of the same size"""
    frames, kw, want, ks = _batch_fit_case()
    H, W = ppr.BATCH_SHAPE
    with sg.Prepro(gpu_ctx, W, H, 1, **kw) as pp:
        assert pp.info().ihot > 0
        rc1, one, k1 = _prepro(gpu_ctx, pp, frames[:1], gap)
        rc, got, k = _prepro(gpu_ctx, pp, frames, gap)
        assert rc == 0 and rc1 == 0, gpu_ctx.error()
        assert k.tobytes() == ks.tobytes(), np.flatnonzero(k != ks)[:5]
        assert np.array_equal(got, want), np.argwhere(got != want)[:5]
        assert k[128] != k[0] and k[256] != k[0]
        if gap == 0:
            host = frames.copy()
            rch, k_host = gpu_ctx.prepro_frames_host(pp, host)
            assert rch == 0, gpu_ctx.error()
            assert np.array_equal(host, got) and k_host.tobytes() == k.tobytes()
        rc2, again, k2 = _prepro(gpu_ctx, pp, frames[:1], gap)
    assert rc2 == 0 and np.array_equal(again, one) and k2.tobytes() == k1.tobytes()
    assert np.array_equal(one, want[:1]) and k1[0] == ks[0]


@pytest.mark.parametrize("gap", [7, 3])
def test_prepro_129_frames_three_layers(gpu_ctx, gap):
    """offset + dark + flat without the fit; gap 7: the 128-bit body with a scalar tail, gap 3: scalar"""
    N, C, H, W = ppr.BATCH_FRAMES_RGB, 3, 5, 63
    assert ((C * H * W + gap) % 8 == 0) == (gap == 7) and (C * H * W) % 8 != 0
    rng = np.random.default_rng(129)
    off, dark, flat = _masters(rng, C, H, W)
    frames = rng.integers(0, 65536, size=(N, C, H, W)).astype(np.uint16)
    kw = dict(offset=off, dark=dark, flat=flat, normalisation=1234.5678)
    want, _ = ppr.preprocess(frames, **kw)
    with sg.Prepro(gpu_ctx, W, H, C, **kw) as pp:
        rc1, one, _ = _prepro(gpu_ctx, pp, frames[:1], gap)
        rc, got, k = _prepro(gpu_ctx, pp, frames, gap)
        rc2, again, _ = _prepro(gpu_ctx, pp, frames[:1], gap)
    assert rc == 0 and rc1 == 0 and rc2 == 0, gpu_ctx.error()
    assert np.array_equal(got, want), np.argwhere(got != want)[:5]
    assert not np.array_equal(want[128], frames[128]) and (k == 1.0).all()
    assert np.array_equal(one, want[:1]) and np.array_equal(again, one)


# ------------------------------------------------------------------ candidates past the first 64

MAX_STARS = [256, 100, 65, 64, 63]


def _dense_refs():
    """the dense frame's fits once (all variants); the reference of every max_stars is their cap_stars"""
    img = pr.starfit_dense_frame()
    r = pr.DENSE_CASE[6]
    cands, want, base = gs._ref(img, r, K, None, 256, 0.5, 65535.0, (1.0, 1.0), MAX_STARS[0])
    assert len(cands) < MAX_STARS[0]            # nothing capped: base["fits"] are all the fits
    for m in MAX_STARS[1:]:
        key = (img.tobytes(), img.shape, r, K, None, 256, 0.5, 65535.0, (1.0, 1.0), m)
        if key not in gs._refs:
            records, stable, stars = pr.cap_stars(*base["fits"], m)
            gs._refs[key] = (cands, want, dict(base, records=records, stable=stable, stars=stars))
    return img, r


@pytest.mark.parametrize("max_stars", MAX_STARS)
def test_star_list_across_candidate_steps(gpu_ctx, max_stars):
    """161 stored candidates, all accepted: the rank of a star carries over the steps of 64 candidates,
    and the cap falls in the third step (256: nowhere), the second (100, 65), on the boundary (64) and
    in the first (63)"""
    img, r = _dense_refs()
    rc, rec, nstars, st, cd = _call(gpu_ctx, img[None, None], r, maxc=256, max_stars=max_stars)
    assert rc == 0, gpu_ctx.error()
    (cands, _, tail), stable = _check_frame(img, rec[0], nstars[0], st[0], cd[0], r, maxc=256, max_stars=max_stars)
    ns = rec[0].nstored
    assert ns == len(cands) >= 129 and stable[:ns].all()
    accepted = [i for i in range(ns) if tail["fits"][0][i]["status"] == pr.FIT_STAR]
    kept = accepted[:max_stars]
    assert nstars[0] == len(kept) == min(max_stars, len(accepted))
    assert st[0]["cand"][:nstars[0]].tolist() == sorted(kept, key=lambda i: (float(cd[0]["mag"][i]), i))
    status = cd[0]["status"][:ns]
    assert (status[kept] == sg.SG_FIT_STAR).all() and (status[accepted[max_stars:]] == sg.SG_FIT_OVER_CAP).all()
    # without the candidate records the stars are the same
    rc, rec2, nstars2, st2, _ = _call(gpu_ctx, img[None, None], r, maxc=256, max_stars=max_stars, want_cands=False)
    assert rc == 0 and nstars2[0] == nstars[0] and st2.tobytes() == st.tobytes() and bytes(rec2[0]) == bytes(rec[0])


# ------------------------------------------------------------------ second sweep of a capped grid

def _big_calibration(gpu_ctx, H, W, gap, subset, seed):
    rng = np.random.default_rng(seed)
    off, dark, flat = _masters(rng, 1, H, W)
    use = dict(offset=off if subset & 1 else None, dark=dark if subset & 2 else None, flat=flat if subset & 4 else None)
    frames = rng.integers(0, 65536, size=(2, 1, H, W)).astype(np.uint16)
    with sg.Prepro(gpu_ctx, W, H, 1, normalisation=1234.5678, **use) as pp:
        rc, got, k = _prepro(gpu_ctx, pp, frames, gap)
    assert rc == 0, gpu_ctx.error()
    want, _ = ppr.preprocess(frames, normalisation=1234.5678, **use)
    assert np.array_equal(got, want), (np.argwhere(got != want)[:5], int((got != want).sum()))
    assert (want == 0).any() and ((want == 65535).any() or not subset & 4)      # saturates
    assert not np.array_equal(want[:, :, -1], frames[:, :, -1])                # the last row is calibrated too


@pytest.mark.parametrize("subset", [7, 2])
def test_calibration_second_sweep_of_the_128_bit_body(gpu_ctx, subset):
    """8 407 050 samples a frame: 1 050 881 vectors of 8 for 4096 x 256 threads, and a tail of 2"""
    H, W, gap = ppr.SWEEP_VECTOR
    assert (H * W + gap) % 8 == 0 and (H * W) % 8 == 2
    _big_calibration(gpu_ctx, H, W, gap, subset, 2050 + subset)


def test_calibration_second_sweep_of_the_scalar_loop(gpu_ctx):
    H, W, gap = ppr.SWEEP_SCALAR
    assert (H * W + gap) % 8 != 0
    _big_calibration(gpu_ctx, H, W, gap, 7, 1025)


def test_no_wavelet_plane_second_sweep_and_capacity(gpu_ctx):
    """31 x 8500: k_findstar_copy's 1024 blocks sweep twice; about 21 800 candidates for 2000 slots"""
    H, W = fr.COPY_SWEEP_SHAPE
    img = fr.tie_image(seed=5, H=H, W=W)
    rc, rec, xy, bx, wave = _find(gpu_ctx, img[None, None], 3, 1.0, maxc=2000)
    assert rc == 0, gpu_ctx.error()
    assert rec[0].wavelet_applied == 0 and np.array_equal(wave[0], img), np.argwhere(wave[0] != img)[:5]
    cands, want, _ = fr.candidates(img, 1.0, 3)
    assert len(cands) > 2000
    _check_record(rec[0], want, len(cands), 2000)
    assert xy[0].tolist() == [list(c) for c in cands[:2000]]
    assert np.array_equal(bx[0], fr.boxes(img, cands[:2000], 3))
