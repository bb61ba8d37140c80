"""Fitted stars on the device (sg_findstar_fit*) against tests/psf_ref.py, the numpy restatement of
the second half of peaker: the start values and candidates bit for bit; status, iterations and the
fitted fields within psf_ref.TOL on branch-stable boxes (a legal status and unchanged start values
on the others); the star list, its order and its caps; frame strides, layers, an empty frame and an
area; norm 255 and FWHM scales; run-to-run identity; the host entry and the refused arguments.
tests/test_psf_cpu.py holds, for the same cases, the share of unstable boxes, the count of stable
stars and the measured spread behind TOL."""
import ctypes

import numpy as np
import pytest

import findstar_ref as fsr
import psf_ref as pr
import sirilgpu as sg

pytestmark = pytest.mark.gpu

GAP_FILL = 0xABCD
BYTE_FILL = 0x5A
K = pr.K_SIGMA


def _filled(n, dtype):
    a = np.empty(n, dtype=dtype)
    a.view(np.uint8)[:] = BYTE_FILL
    return a


def _untouched(a):
    return bool((np.ascontiguousarray(a).view(np.uint8) == BYTE_FILL).all())


def _call(ctx, frames, r, k=K, layer=0, area=None, maxc=64, gap=0, roundness=0.5, norm=65535.0, scales=(1.0, 1.0),
          max_stars=64, want_cands=True, host=False, desc_edit=None):
    """sg_findstar_fit_device (or sg_findstar_fit) on frames [N][C][H][W], C*H*W + gap samples apart,
    into guarded arrays.  The frames, the gaps and the guards after every output array must come back
    untouched, as must every slot past a frame's counts.
    Returns (rc, records, nstars[N], stars[N][max_stars], cands[N][maxc])."""
    import torch
    N, C, H, W = frames.shape
    total = C * H * W
    stride = total + gap
    d = sg.make_starfit_desc(W, H, C, layer, r, k, area, maxc, roundness, norm, scales, max_stars, want_cands)
    if desc_edit:
        desc_edit(d)
    rec = (sg.FindstarFrame * (N + 1))()
    ctypes.memset(rec, BYTE_FILL, ctypes.sizeof(rec))
    nstars = _filled(N + 8, np.int32)
    stars = _filled(N * max(max_stars, 0) + 2, sg.STAR_DTYPE)
    cands = _filled(N * max(maxc, 0) + 2, sg.CAND_DTYPE)
    P = ctypes.c_void_p
    if host:
        rc = ctx.lib.sg_findstar_fit(ctx.ctx, ctypes.byref(d), np.ascontiguousarray(frames).ctypes.data_as(P), N, rec,
                                     nstars.ctypes.data_as(P), stars.ctypes.data_as(P),
                                     cands.ctypes.data_as(P) if want_cands else None)
    else:
        buf = np.full(N * stride + 64, GAP_FILL, dtype=np.uint16)
        for i in range(N):
            buf[i * stride:i * stride + total] = frames[i].reshape(-1)
        dev = torch.from_numpy(buf.view(np.int16).copy()).cuda()
        torch.cuda.synchronize()
        rc = ctx.lib.sg_findstar_fit_device(ctx.ctx, 0, ctypes.byref(d), P(dev.data_ptr()), N, stride if gap else 0, rec,
                                            nstars.ctypes.data_as(P), stars.ctypes.data_as(P),
                                            cands.ctypes.data_as(P) if want_cands else None, None)
        torch.cuda.synchronize()
        assert np.array_equal(dev.cpu().numpy().view(np.uint16), buf), "the frames, a gap or the guard changed"
    assert _untouched(nstars[N:]) and _untouched(stars[N * max(max_stars, 0):]) and _untouched(cands[N * max(maxc, 0):])
    assert bytes(rec[N]) == bytes([BYTE_FILL]) * ctypes.sizeof(sg.FindstarFrame), "guard after the records written"
    if rc != 0:
        assert _untouched(nstars) and _untouched(stars) and _untouched(cands), "a refused call wrote an output"
        assert bytes(rec) == bytes([BYTE_FILL]) * ctypes.sizeof(rec), "a refused call wrote a record"
        return rc, None, None, None, None
    st = stars[:N * max_stars].reshape(N, max_stars)
    cd = cands[:N * maxc].reshape(N, maxc)
    for f in range(N):
        assert 0 <= nstars[f] <= max_stars
        assert _untouched(st[f, nstars[f]:]), "a star slot past nstars written"
        assert _untouched(cd[f, rec[f].nstored if want_cands else 0:]), "a candidate slot past nstored written"
    return rc, list(rec)[:N], nstars[:N].copy(), st, cd


_refs = {}


def _ref(plane, r, k, area, maxc, roundness, norm, scales, max_stars):
    """(candidates, threshold record, peaker_tail of the stored ones), computed once per case"""
    key = (plane.tobytes(), plane.shape, r, k, area, maxc, roundness, norm, scales, max_stars)
    if key not in _refs:
        cands, rec, _ = fsr.candidates(plane, k, r, area)
        tail = pr.peaker_tail(plane, cands[:maxc], r, rec["median"], roundness, norm, scales, max_stars,
                              variants=pr.ALL_VARIANTS)
        _refs[key] = (cands, rec, tail)
    return _refs[key]


def _close(a, b):
    a, b = float(a), float(b)
    return (np.isnan(a) and np.isnan(b)) or a == b or abs(a - b) <= pr.TOL * max(abs(b), 1.0)


def _check_frame(plane, q, n, st, cd, r, k=K, area=None, maxc=64, roundness=0.5, norm=65535.0, scales=(1.0, 1.0),
                 max_stars=64):
    """one frame's whole answer against the restatement; returns (reference, stable mask)"""
    cands, want, tail = _ref(plane, r, k, area, maxc, roundness, norm, scales, max_stars)
    assert q.ngood == want["ngood"] and q.no_data == want["no_data"] and q.threshold == want["threshold"]
    assert q.ncand == len(cands) and q.nstored == min(len(cands), maxc)
    ns = q.nstored
    stable, recs = tail["stable"], tail["records"]
    worst = max([abs(float(cd[name][i]) - float(recs[i][name])) / max(abs(float(recs[i][name])), 1.0)
                 for i in range(ns) if stable[i] and recs[i]["status"] in (pr.FIT_STAR, pr.FIT_NOT_STAR, pr.FIT_OVER_CAP)
                 for name in pr.FIELDS if np.isfinite(recs[i][name]) and np.isfinite(cd[name][i])], default=0.0)
    print(f"r {r} candidates {ns} unstable {int((~stable[:ns]).sum())}: largest relative difference {worst:.3e}, "
          f"TOL {pr.TOL:.3e}")
    assert cd["x"][:ns].tolist() == [c[0] for c in cands[:ns]] and cd["y"][:ns].tolist() == [c[1] for c in cands[:ns]]
    for i in range(ns):
        w = recs[i]
        assert cd["init"][i].tobytes() == w["init"].tobytes(), (i, cd["init"][i], w["init"])
        assert 0 <= cd["status"][i] <= sg.SG_FIT_OVER_CAP and cd["reserved"][i] == 0
        if not stable[i]:
            continue
        assert (cd["status"][i], cd["failed_test"][i], cd["iters"][i]) == (w["status"], w["failed_test"], w["iters"]), \
            (i, cd[i], w["status"], w["failed_test"], w["iters"])
        if w["status"] in (pr.FIT_STAR, pr.FIT_NOT_STAR, pr.FIT_BAD_FWHM, pr.FIT_OVER_CAP):
            for name in pr.FIELDS:
                assert _close(cd[name][i], w[name]), (i, name, cd[name][i], w[name])
    # the star list: the first max_stars accepted in candidate order, sorted by (mag, cand), each the copy
    # of its candidate record
    accepted = [i for i in range(ns) if cd["status"][i] in (sg.SG_FIT_STAR, sg.SG_FIT_OVER_CAP)]
    kept = accepted[:max_stars]
    assert n == len(kept) and all(cd["status"][i] == sg.SG_FIT_OVER_CAP for i in accepted[max_stars:])
    assert all(cd["status"][i] == sg.SG_FIT_STAR for i in kept)
    got = st[:n]
    assert sorted(got["cand"].tolist()) == kept
    order = sorted(range(n), key=lambda i: (float(got["mag"][i]), int(got["cand"][i])))
    assert order == list(range(n)), "the star list is not sorted by (mag, cand)"
    for s in got:
        c = cd[s["cand"]]
        assert (s["x"], s["y"], s["iters"]) == (c["x"], c["y"], c["iters"])
        assert all(s[name].tobytes() == c[name].tobytes() for name in pr.FIELDS)
    if stable[:ns].all() or len(accepted) <= max_stars:
        assert [int(c) for c in got["cand"] if stable[c]] == [i for i in tail["stars"] if stable[i]]
    return (cands, want, tail), stable


# ------------------------------------------------------------------ box size and lane count

@pytest.mark.parametrize("r", sorted(pr.STARFIT_CASES))
def test_box_sizes(gpu_ctx, r):
    """n = 16, 36, 64, 100, 400, 1024, 4096 pixels: less than a wave, exactly a wave, no multiple of 64,
    the default and the limit; a star r from the border, a hot pixel beside a star, a clipped star"""
    img = pr.starfit_frame(r)
    rc, rec, nstars, st, cd = _call(gpu_ctx, img[None, None], r)
    assert rc == 0, gpu_ctx.error()
    (cands, _, tail), stable = _check_frame(img, rec[0], nstars[0], st[0], cd[0], r)
    assert rec[0].nstored == len(cands) >= 30
    assert sum(1 for i in tail["stars"] if stable[i]) >= 10 and nstars[0] >= 10


def test_radius_1_has_too_few_pixels(gpu_ctx):
    img = pr.starfit_frame(2)
    rc, rec, nstars, st, cd = _call(gpu_ctx, img[None, None], 1, maxc=256)
    assert rc == 0, gpu_ctx.error()
    assert rec[0].nstored > 0 and nstars[0] == 0
    assert (cd[0]["status"][:rec[0].nstored] == sg.SG_FIT_NOT_ENOUGH_PIXELS).all()
    assert (cd[0]["iters"][:rec[0].nstored] == 0).all()
    _check_frame(img, rec[0], nstars[0], st[0], cd[0], 1, maxc=256)


# ------------------------------------------------------------------ star list and caps

def test_max_stars_keeps_the_first_in_raster_order(gpu_ctx):
    img = pr.starfit_frame(5)
    rc, rec, nstars, st, cd = _call(gpu_ctx, img[None, None], 5, max_stars=7)
    assert rc == 0, gpu_ctx.error()
    _check_frame(img, rec[0], nstars[0], st[0], cd[0], 5, max_stars=7)
    assert nstars[0] == 7 and (cd[0]["status"][:rec[0].nstored] == sg.SG_FIT_OVER_CAP).sum() >= 10
    rc, rec, nstars, st, cd = _call(gpu_ctx, img[None, None], 5, max_stars=0)
    assert rc == 0 and nstars[0] == 0 and rec[0].nstored >= 30


def test_max_candidates_below_ncand(gpu_ctx):
    img = pr.starfit_frame(5)
    rc, rec, nstars, st, cd = _call(gpu_ctx, img[None, None], 5, maxc=12)
    assert rc == 0, gpu_ctx.error()
    assert rec[0].ncand >= 30 and rec[0].nstored == 12
    _check_frame(img, rec[0], nstars[0], st[0], cd[0], 5, maxc=12)
    assert nstars[0] <= 12 and (st[0]["cand"][:nstars[0]] < 12).all()
    # without the candidate records the stars are the same
    rc, rec2, nstars2, st2, _ = _call(gpu_ctx, img[None, None], 5, maxc=12, want_cands=False)
    assert rc == 0 and nstars2[0] == nstars[0] and st2.tobytes() == st.tobytes()


# ------------------------------------------------------------------ layout

def test_three_frames_gap_stride_layer_and_empty_frame(gpu_ctx):
    r = 5
    a = pr.starfit_frame(r)
    b = np.ascontiguousarray(a[::-1, ::-1])
    H, W = a.shape
    frames = np.random.default_rng(3).integers(0, 3000, size=(3, 3, H, W)).astype(np.uint16)
    frames[0, 1], frames[2, 1] = a, b
    frames[1] = 0
    rc, rec, nstars, st, cd = _call(gpu_ctx, frames, r, layer=1, gap=37)
    assert rc == 0, gpu_ctx.error()
    _check_frame(a, rec[0], nstars[0], st[0], cd[0], r)
    _check_frame(b, rec[2], nstars[2], st[2], cd[2], r)
    assert rec[1].no_data == 1 and rec[1].ncand == 0 and rec[1].nstored == 0 and nstars[1] == 0
    assert nstars[0] >= 10 and nstars[2] >= 10


def test_use_area(gpu_ctx):
    r = 10
    img = pr.starfit_frame(r)
    area = (9, 13, 101, 97)
    rc, rec, nstars, st, cd = _call(gpu_ctx, img[None, None], r, area=area)
    assert rc == 0, gpu_ctx.error()
    (cands, _, _), _ = _check_frame(img, rec[0], nstars[0], st[0], cd[0], r, area=area)
    full = fsr.candidates(img, K, r)[0]
    assert 5 <= len(cands) < len(full)
    assert all(area[0] + r <= x < area[0] + area[2] - r and area[1] + r <= y < area[1] + area[3] - r for x, y in cands)


# ------------------------------------------------------------------ parameters

def test_norm_255(gpu_ctx):
    img = pr.starfit_frame(10)
    rc, rec, nstars, st, cd = _call(gpu_ctx, img[None, None], 10, norm=255.0)
    assert rc == 0, gpu_ctx.error()
    _check_frame(img, rec[0], nstars[0], st[0], cd[0], 10, norm=255.0)
    assert nstars[0] >= 10 and (st[0]["A"][:nstars[0]] > 1.0).any()      # normalised by 255, not 65535


def test_fwhm_scales_flip_a_roundness_decision(gpu_ctx):
    img = pr.starfit_frame(10)
    kw = dict(roundness=0.7, scales=(1.0, 0.62))
    rc, rec, nstars, st, cd = _call(gpu_ctx, img[None, None], 10, **kw)
    assert rc == 0, gpu_ctx.error()
    (_, _, tail), stable = _check_frame(img, rec[0], nstars[0], st[0], cd[0], 10, **kw)
    rc, rec1, nstars1, st1, cd1 = _call(gpu_ctx, img[None, None], 10, roundness=0.7)
    assert rc == 0, gpu_ctx.error()
    (_, _, tail1), stable1 = _check_frame(img, rec1[0], nstars1[0], st1[0], cd1[0], 10, roundness=0.7)
    flipped = [i for i in range(rec[0].nstored) if stable[i] and stable1[i] and
               tail1["records"][i]["status"] == pr.FIT_STAR and tail["records"][i]["status"] == pr.FIT_NOT_STAR and
               tail["records"][i]["failed_test"] == 8]
    assert flipped and all(cd[0]["status"][i] == sg.SG_FIT_NOT_STAR and cd1[0]["status"][i] == sg.SG_FIT_STAR
                           for i in flipped)


# ------------------------------------------------------------------ run to run, entry points

def test_two_calls_return_identical_bytes(gpu_ctx):
    img = pr.starfit_frame(16)
    a = _call(gpu_ctx, img[None, None], 16)
    b = _call(gpu_ctx, img[None, None], 16)
    assert a[0] == 0 and b[0] == 0
    assert a[2].tobytes() == b[2].tobytes() and a[3].tobytes() == b[3].tobytes() and a[4].tobytes() == b[4].tobytes()


def test_host_entry_equals_device_entry(gpu_ctx):
    r = 5
    a = pr.starfit_frame(r)
    frames = np.stack([a, np.ascontiguousarray(a[::-1])])[:, None]
    dev = _call(gpu_ctx, frames, r)
    host = _call(gpu_ctx, frames, r, host=True)
    assert dev[0] == 0 and host[0] == 0, gpu_ctx.error()
    assert dev[2].tobytes() == host[2].tobytes() and dev[3].tobytes() == host[3].tobytes()
    assert dev[4].tobytes() == host[4].tobytes() and [bytes(q) for q in dev[1]] == [bytes(q) for q in host[1]]
    # the binding's own calls return the same records
    rc, rec, nstars, st, cd = gpu_ctx.findstar_fit(frames, r, K, max_candidates=64, max_stars=64, want_candidates=True)
    assert rc == 0 and nstars.tobytes() == dev[2].tobytes()
    for f in range(2):
        assert st[f, :nstars[f]].tobytes() == dev[3][f, :nstars[f]].tobytes()
        assert cd[f, :rec[f].nstored].tobytes() == dev[4][f, :rec[f].nstored].tobytes()


def _set(**kw):
    def edit(d):
        for name, v in kw.items():
            obj = d.find if name in ("layer", "radius", "width", "sigma", "max_candidates") else d
            setattr(obj, name, v)
    return edit


REFUSED = [
    (dict(radius=33), sg.SG_ERR_GENERIC), (dict(roundness=float("nan")), sg.SG_ERR_GENERIC),
    (dict(roundness=float("inf")), sg.SG_ERR_GENERIC), (dict(fwhm_scale_x=float("inf")), sg.SG_ERR_GENERIC),
    (dict(fwhm_scale_y=float("nan")), sg.SG_ERR_GENERIC), (dict(norm=1000.0), sg.SG_ERR_GENERIC),
    (dict(norm=65536.0), sg.SG_ERR_GENERIC), (dict(max_stars=-1), sg.SG_ERR_GENERIC),
    (dict(max_stars=50001), sg.SG_ERR_GENERIC), (dict(layer=1), sg.SG_ERR_SIZE), (dict(width=0), sg.SG_ERR_SIZE),
    (dict(radius=0), sg.SG_ERR_GENERIC), (dict(sigma=-1.0), sg.SG_ERR_GENERIC),
    (dict(max_candidates=-1), sg.SG_ERR_GENERIC),
]


def test_refused_arguments_touch_nothing(gpu_ctx):
    img = pr.starfit_frame(5)
    for kw, code in REFUSED:
        for host in (False, True):
            rc = _call(gpu_ctx, img[None, None], 5, host=host, desc_edit=_set(**kw))[0]     # asserts the outputs untouched
            assert rc == code, (kw, host, rc)
            assert gpu_ctx.error()


def test_findstar_device_is_unchanged(gpu_ctx):
    """the candidate call on the same frames still returns what it did: list, records and boxes"""
    import torch
    r = 5
    img = pr.starfit_frame(r)
    d = torch.from_numpy(img.view(np.int16).copy()).cuda()
    torch.cuda.synchronize()
    H, W = img.shape
    rc, rec, xy, bx = gpu_ctx.findstar_device(d.data_ptr(), 1, 1, H, W, r, K, max_candidates=64)
    assert rc == 0, gpu_ctx.error()
    cands, want, _ = fsr.candidates(img, K, r)
    n = len(cands)
    assert rec[0].ncand == n and rec[0].threshold == want["threshold"] and xy[0, :n].tolist() == [list(c) for c in cands]
    assert np.array_equal(bx[0, :n], fsr.boxes(img, cands, r)) and (bx[0, n:] == 0).all() and (xy[0, n:] == 0).all()
    rc, rec2, nstars, st, cd = gpu_ctx.findstar_fit_device(d.data_ptr(), 1, 1, H, W, r, K, max_candidates=64, max_stars=64,
                                                           want_candidates=True)
    assert rc == 0 and bytes(rec2[0]) == bytes(rec[0])
    assert cd["x"][0, :n].tolist() == [c[0] for c in cands] and cd["y"][0, :n].tolist() == [c[1] for c in cands]
