"""What tests/test_gpu_batches.py relies on, held without a GPU: the chunk sizes of the resident-frame
entries (read from the sources, so a retuned chunk fails here and not silently there) against the frame
counts of the cases, the sample counts of the large frames against the caps of the two capped grids,
the candidate counts of the dense PSF frame per 64-candidate step, the different fitted k of the chunks'
first frames, and the many-frame sequences themselves."""
import os
import re
import subprocess

import numpy as np

import findstar_ref as fr
import prepro_ref as ppr
import psf_ref as pr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "siril-0.9_amd", "csrc")

PROGRAM = r'''
#include <stdio.h>
#include <string.h>
#include <stdlib.h>
#include "sg_findstar_plan.hpp"

int main(int argc, char **argv) {
	sg_findstar_desc d;
	memset(&d, 0, sizeof d);
	d.nb_layers = 1;
	d.radius = 3;
	d.sigma = 1.0;
	d.max_candidates = 10;
	for (int i = 1; i + 2 < argc; i += 3) {
		SgFindstarPlan p;
		d.height = atoi(argv[i]);
		d.width = atoi(argv[i + 1]);
		if (sg_findstar_plan(&d, p) != SG_OK)
			return 1;
		const int n = atoi(argv[i + 2]);
		printf("%d %d %d\n", sgf_chunk_frames(p, n, 1), sgf_chunk_frames(p, n, 0), p.wavelet);
	}
	return 0;
}
'''


def _source(name):
    with open(os.path.join(SRC, name)) as f:
        return f.read()


def _one(pattern, text):
    found = re.findall(pattern, text)
    assert len(found) == 1, (pattern, found)
    return int(found[0])


def test_findstar_chunks_against_the_frame_counts(tmp_path):
    """sgf_chunk_frames of the cases' shapes, with and without the caller's plane array: every case has one
    full chunk and a second of one or two frames"""
    src = tmp_path / "chunks.cpp"
    src.write_text(PROGRAM)
    exe = tmp_path / "chunks"
    r = subprocess.run(["g++", "-O1", "-std=c++17", "-I", SRC, str(src), "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    fit_shape = pr.starfit_frame(5).shape
    cases = [(fr.BATCH_SHAPE, n) for n in fr.BATCH_FRAMES] + [(fit_shape, n) for n in fr.BATCH_FRAMES]
    args = [str(v) for (H, W), n in cases for v in (H, W, n)]
    out = subprocess.run([str(exe), *args], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    rows = [[int(v) for v in line.split()] for line in out.stdout.splitlines()]
    assert len(rows) == len(cases)
    for (shape, n), (with_plane, without, wavelet) in zip(cases, rows):
        assert with_plane == without and wavelet == 1
        assert n - with_plane in (1, 2), (shape, n, with_plane)
    assert sorted(n - row[0] for (_, n), row in zip(cases, rows)) == [1, 1, 2, 2]


def test_prepro_chunks_against_the_frame_counts():
    chunk = _one(r"#define SGP_CHUNK_FRAMES (\d+)", _source("sg_prepro.hip"))
    assert ppr.BATCH_FRAMES == 2 * chunk + 1            # frames 128 and 256 open the second and third chunk
    assert ppr.BATCH_FRAMES_RGB == chunk + 1
    # the host entry's batch is the same number for small frames: the shared loop capped by the chunk
    # (tests/test_host_batch_cpu.py pins the rule: 257 frames of this shape under that cap go 128 at a time)
    assert "hb.begin(nframes, total, SG_HOST_BUDGET_1G, SGP_CHUNK_FRAMES)" in _source("sg_prepro.hip")


def test_large_frames_pass_the_capped_grids():
    blocks = _one(r"std::min<int64_t>\(\(units \+ 255\) / 256, (\d+)\)", _source("sg_prepro.hip"))
    H, W, gap = ppr.SWEEP_VECTOR
    assert (H * W) >> 3 > blocks * 256 and (H * W) % 8 != 0 and (H * W + gap) % 8 == 0
    assert (H * W) >> 3 < 2 * blocks * 256              # the smallest that does: one more sweep, not several
    H, W, gap = ppr.SWEEP_SCALAR
    assert blocks * 256 < H * W < 2 * blocks * 256 and (H * W + gap) % 8 != 0
    blocks = _one(r"std::min<int64_t>\(\(npix \+ 255\) / 256, (\d+)\)", _source("sg_findstar.hip"))
    H, W = fr.COPY_SWEEP_SHAPE
    assert blocks * 256 < H * W < 2 * blocks * 256 and min(H, W) < fr.MIN_SIDE


def test_dense_frame_fills_three_candidate_steps():
    """at least 129 stored candidates, none unstable, at least 10 accepted in each step of 64; and cap_stars
    of the uncapped fits is peaker_tail with that cap"""
    img = pr.starfit_dense_frame()
    seed, H, W, gx, gy, fwhm, r = pr.DENSE_CASE
    assert img.shape == (H, W) == (192, 192)
    cands, rec, _ = fr.candidates(img, pr.K_SIGMA, r)
    assert 129 <= len(cands) <= 192
    tail = pr.peaker_tail(img, cands[:256], r, rec["median"], max_stars=256, variants=pr.ALL_VARIANTS)
    assert tail["stable"].all()
    accepted = [i for i, o in enumerate(tail["records"]) if o["status"] == pr.FIT_STAR]
    per_step = [sum(1 for i in accepted if s <= i < s + 64) for s in (0, 64, 128)]
    print(f"candidates {len(cands)}, accepted per step {per_step}")
    assert min(per_step) >= 10
    for m in (100, 63):
        records, stable, stars = pr.cap_stars(*tail["fits"], m)
        direct = pr.peaker_tail(img, cands[:256], r, rec["median"], max_stars=m)
        assert [o["status"] for o in records] == [o["status"] for o in direct["records"]]
        assert stars == direct["stars"] and len(stars) == m and stable.all()
        assert sum(1 for o in records if o["status"] == pr.FIT_OVER_CAP) == len(accepted) - m


def test_fit_sequence_planes():
    """frames 255 to 257 are the field, the empty frame and the rotation; both fields accept 7 + 10 stars"""
    frames, which, planes = pr.starfit_batch_sequence(258)
    assert frames.shape == (258, 1, 112, 128) and which[:4] == [0, 1, 2, 0] and which[255:] == [0, 2, 1]
    assert not planes[2].any() and not np.array_equal(planes[0], planes[1])
    assert pr.starfit_batch_sequence(257)[1][255:] == [0, 2]
    for p in planes[:2]:
        cands, rec, _ = fr.candidates(p, pr.K_SIGMA, 5)
        tail = pr.peaker_tail(p, cands[:64], 5, rec["median"])
        assert 30 <= len(cands) <= 64 and len(tail["stars"]) >= 17


def test_candidate_sequences():
    """every star field has candidates, the fourth a list of its own; the empty area scans nothing"""
    frames, which, planes = fr.batch_sequence(258, [-1, 3])
    assert frames.shape == (258, 1) + fr.BATCH_SHAPE and which[253:] == [1, 2, 0, -1, 3]
    assert not frames[256].any() and np.array_equal(frames[257, 0], planes[3])
    lists = [fr.candidates(p, 1.0, 3)[0] for p in planes]
    assert all(len(c) >= 1 for c in lists) and all(lists[3] != c for c in lists[:3])
    x0, x1, y0, y1 = fr.scan_rect(fr.BATCH_SHAPE, 3, fr.BATCH_EMPTY_AREA)
    assert x1 <= x0 and y1 > y0
    assert fr.candidates(planes[0], 1.0, 3, fr.BATCH_EMPTY_AREA)[0] == []


def test_chunks_open_with_a_different_k():
    """the fitted k of frames 0, 128 and 256 differ, so a chunk that read the first chunk's k shows"""
    frames, dark, k_true = ppr.batch_fit_case()
    assert len(k_true) == ppr.BATCH_FRAMES and k_true[0] == 0.2 and k_true[-1] == 1.7
    k = [ppr.search_rule(lambda kk: ppr.objective(frames[i, 0], dark, kk))[0] for i in (0, 128, 256)]
    assert k[1] != k[0] and k[2] != k[0] and k[2] != k[1]
    assert all(abs(a - b) < 0.05 for a, b in zip(k, k_true[[0, 128, 256]]))
