"""The six host-frame entries past one host batch.  They share one batch loop (SgHostBatches in
siril-0.9_amd/csrc/sg_ctx.hpp), which by default batches by the gibibyte, so no test of ordinary
size reaches a second batch; SG_HOST_BATCH caps the batch in frames.  Every case here takes 5 frames
(quality: 6 included ones of 7) on a context created under SG_HOST_BATCH=2, so the batches are
2 + 2 + 1, and must return, byte for byte, what the same host entry returns on the default context
in one batch, which the tests of each entry tie to the oracles.  The frames of a case differ from
one another, so a wrong offset of a later batch into the frames or into a result array shows.

A library that ignored the knob would pass the five comparisons in one batch each.  What keeps them
from being vacuous are the two launch counts of sg_quality_last_times asserted below, which only a
library that really splits the batches reports, together with tests/test_host_batch_cpu.py, which
pins the one rule all six entries size their batches by.

The last test's case of 5 frames under SG_HOST_BATCH=3 and SG_QUALITY_CHUNK=2 reports 3 launches
whichever cap holds (3 + 2 frames in chunks of 2 are 2 + 1 launches as well), so 6 frames are run
beside it: 2 + 2 + 2 are 3 launches, 3 + 3 in chunks of 2 would be 4."""
import os

import numpy as np
import pytest

import cosme_cases as cc
import findstar_ref as fr
import prepro_ref as ppr
import psf_ref as pr
import sirilgpu as sg
from test_gpu_ecc import frames_of as ecc_frames
from test_gpu_quality import RESIDENT, _seven

pytestmark = pytest.mark.gpu

N = 5


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
def ctx2(gpu_ctx):
    c = _context(SG_HOST_BATCH=2)
    yield c
    c.close()


def _same(a, b):
    """two results (rc first) are the same bytes: ctypes records, arrays, dicts of arrays, None"""
    assert a[0] == 0 and b[0] == 0 and len(a) == len(b)
    for x, y in zip(a[1:], b[1:]):
        if isinstance(x, list):
            assert [bytes(q) for q in x] == [bytes(q) for q in y]
        elif isinstance(x, dict):
            assert x.keys() == y.keys() and all(x[k].tobytes() == y[k].tobytes() for k in x)
        else:
            assert (x is None) == (y is None) and (x is None or x.tobytes() == y.tobytes())


@pytest.mark.parametrize("want_wave", [True, False])
def test_findstar(gpu_ctx, ctx2, want_wave):
    frames, which, _ = fr.batch_sequence(N, [-1, 3])
    assert frames.shape[2:] == fr.BATCH_SHAPE and len(set(which)) == N
    kw = dict(max_candidates=10, want_boxes=True, want_wave=want_wave)
    one = gpu_ctx.findstar(frames, 3, 1.0, **kw)
    got = ctx2.findstar(frames, 3, 1.0, **kw)
    assert got[0] == 0, ctx2.error()
    _same(one, got)
    assert (got[4] is not None) == want_wave
    assert all(got[1][f].nstored >= 1 for f in (0, 1, 2, 4)) and got[2][4].tolist() != got[2][0].tolist()


def test_findstar_fit(gpu_ctx, ctx2):
    a = pr.starfit_frame(5)
    frames = np.stack([a, a[::-1], a[:, ::-1], np.zeros_like(a), a[::-1, ::-1]])[:, None]
    kw = dict(max_candidates=64, max_stars=64, want_candidates=True)
    one = gpu_ctx.findstar_fit(frames, 5, pr.K_SIGMA, **kw)
    got = ctx2.findstar_fit(frames, 5, pr.K_SIGMA, **kw)
    assert got[0] == 0, ctx2.error()
    _same(one, got)
    assert got[2].tolist()[3] == 0 and all(got[2][f] >= 10 for f in (0, 1, 2, 4))
    assert got[3][4].tobytes() != got[3][0].tobytes()


def test_prepro_frames_host(gpu_ctx, ctx2):
    H, W = ppr.BATCH_SHAPE
    k_true = np.array([0.3, 0.65, 1.0, 1.35, 1.7])
    frames, dark = ppr.fit_case(H, W, k_true, seed=H + W)
    off = np.random.default_rng(5).integers(90, 110, size=(1, H, W)).astype(np.uint16)
    kw = dict(offset=off, dark=dark[None], dark_optimization=True, cosmetic=True, cosme_sigma=(3.0, 3.0))
    res = []
    for ctx in (gpu_ctx, ctx2):
        with sg.Prepro(ctx, W, H, 1, **kw) as pp:
            assert pp.info().ihot > 0
            host = frames.copy()
            rc, k = ctx.prepro_frames_host(pp, host)
            assert rc == 0, ctx.error()
            res.append((rc, host, k))
    _same(*res)
    k = res[1][2]
    assert len(set(k.tolist())) == N and np.abs(k - k_true).max() < 0.05
    assert not np.array_equal(res[1][1], frames)


def test_cosme_autodetect(gpu_ctx, ctx2):
    c = cc.CASES["s_1x7"]
    frames = np.concatenate([cc._small(1, 7, seed) for seed in range(N)])
    assert frames.shape == (N,) + cc.frames_of("s_1x7").shape[1:] and len({f.tobytes() for f in frames}) == N
    res = []
    for ctx in (gpu_ctx, ctx2):
        host = frames.copy()
        rc, rec = ctx.cosme_autodetect(host, sig=c["sig"], amount=c["amount"], is_cfa=c["is_cfa"])
        assert rc == 0, ctx.error()
        res.append((rc, rec, host))
    _same(*res)
    assert len({bytes(r) for r in res[1][1]}) > 1


def test_register_ecc_reference_alone_in_the_last_batch(gpu_ctx, ctx2):
    frames = ecc_frames(37, 61, 1, ref_at=4)[:N]
    inc = np.array([1, 0, 1, 1, 1], dtype=np.int32)
    one = gpu_ctx.register_ecc(frames, ref_image=4, included=inc)
    got = ctx2.register_ecc(frames, ref_image=4, included=inc)
    assert got[0] == 0, ctx2.error()
    _same(one, got)
    res = got[1]
    assert all(res["iterations"][f] > 0 for f in (0, 2, 3)) and res["iterations"][1] == 0 and res["iterations"][4] == 0
    assert len({(int(res["shiftx"][f]), int(res["shifty"][f])) for f in (0, 2, 3)}) == 3


def test_quality_launches_are_summed_over_the_batches(gpu_ctx, ctx2):
    fr7 = _seven()
    inc = [1, 0, 1, 1, 1, 1, 1]
    one = gpu_ctx.quality(fr7, included=inc, fill=-1.5)
    assert one[0] == 0, gpu_ctx.error()
    assert gpu_ctx.quality_last_times()[1:] == (RESIDENT, 1)
    got = ctx2.quality(fr7, included=inc, fill=-1.5)
    assert got[0] == 0, ctx2.error()
    _same(one, got)
    assert ctx2.quality_last_times()[1:] == (RESIDENT, 3)      # batches of 2 + 2 + 2, one launch each
    assert got[1][1] == -1.5 and len(set(got[1].tolist())) == 7


def test_the_smaller_cap_wins(gpu_ctx):
    fr7 = _seven()
    one = gpu_ctx.quality(fr7)
    ctx = _context(SG_HOST_BATCH=3, SG_QUALITY_CHUNK=2)
    try:
        got = ctx.quality(fr7[:N])
        assert got[0] == 0, ctx.error()
        assert got[1].tobytes() == one[1][:N].tobytes()
        assert ctx.quality_last_times()[1:] == (RESIDENT, 3)      # 2 + 2 + 1
        got = ctx.quality(fr7[:6])
        assert got[0] == 0, ctx.error()
        assert got[1].tobytes() == one[1][:6].tobytes()
        assert ctx.quality_last_times()[1:] == (RESIDENT, 3)      # 2 + 2 + 2; batches of 3 + 3 would launch 4 times
    finally:
        ctx.close()
