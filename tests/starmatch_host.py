"""The stand-alone host program around siril-0.9_amd/csrc/sg_starmatch.h and sg_starmatch_plan.hpp (what
sg_starmatch runs, with nlanes = 1 and the workspace on the heap), its build and its file formats; shared by
tests/test_starmatch_cpu.py and tests/test_gpu_starmatch.py."""
import os
import struct
import subprocess

import numpy as np

import starmatch_ref as sr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INC = os.path.join(ROOT, "siril-0.9_amd", "csrc")
FIT_FIELDS = ("B", "A", "x0", "y0", "sx", "sy", "fwhmx", "fwhmy", "mag", "rmse", "xpos", "ypos")
STAR_DTYPE = np.dtype([("cand", "<i4"), ("x", "<i4"), ("y", "<i4"), ("iters", "<i4")] + [(k, "<f8") for k in FIT_FIELDS])
SAN = ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan"]

PROGRAM = r'''
#include <stdio.h>
#include <stdlib.h>
#include <stdint.h>
#include <string.h>
#include <time.h>
#include <vector>
#include "sg_starmatch_plan.hpp"

/* input: int32 nframes, max_stars, ref_image, has_included; uint8 included[nframes] if has_included;
 * int32 nstars[nframes]; sg_star stars[nframes][max_stars].  Output: the plan's return code and message,
 * then per frame the integer fields, the fp fields as hex floats and the pairs, then the warp plan.
 * Every buffer is on the heap and exactly sized: the sanitizer sees an index past either end. */
int main(int argc, char **argv) {
	if (argc < 2)
		return 2;
	FILE *fi = fopen(argv[1], "rb");
	if (!fi)
		return 2;
	int32_t h[4];
	if (fread(h, 4, 4, fi) != 4)
		return 2;
	const int nframes = h[0], max_stars = h[1], ref = h[2];
	std::vector<uint8_t> inc((size_t)(nframes > 0 ? nframes : 0));
	if (h[3] && fread(inc.data(), 1, inc.size(), fi) != inc.size())
		return 2;
	std::vector<int32_t> nstars((size_t)(nframes > 0 ? nframes : 0));
	if (fread(nstars.data(), 4, nstars.size(), fi) != nstars.size())
		return 2;
	std::vector<sg_star> stars(nstars.size() * (size_t)(max_stars > 0 ? max_stars : 0));
	if (fread(stars.data(), sizeof(sg_star), stars.size(), fi) != stars.size())
		return 2;
	fclose(fi);
	std::vector<sg_starmatch_result> res(nstars.size());
	memset(res.data(), 0x5a, res.size() * sizeof(sg_starmatch_result));
	SgStarmatchPlan pl;
	const int rc = sg_starmatch_plan(nframes, max_stars, nstars.data(), stars.data(), ref, h[3] ? inc.data() : nullptr, res.data(), 1, pl);
	printf("plan %d %zu %u %d %s\n", rc, pl.lds_bytes, pl.grid, pl.nmax, pl.err);
	if (rc != SG_OK)
		return 0;
	std::vector<int32_t> pairs((size_t)nframes * 2 * MAX_STARS_FITTED, -1);
	sgm_fill_unmatched(pl, max_stars, stars.data(), res.data());
	struct timespec t0, t1;
	clock_gettime(CLOCK_MONOTONIC, &t0);
	for (const SgStarmatchItem &it : pl.items) {
		std::vector<unsigned char> mem(sgm_work_bytes(pl.nmax));
		const SgmWork w = sgm_work(mem.data(), pl.nmax);
		std::vector<double> A(pl.packed.begin() + it.a_off, pl.packed.begin() + it.a_off + 3 * (size_t)it.n);
		std::vector<double> B(pl.packed.begin(), pl.packed.begin() + 3 * (size_t)it.n);
		sgm_frame(w, 0, 1, A.data(), B.data(), it.n, &res[(size_t)it.frame], pairs.data() + (size_t)it.frame * 2 * MAX_STARS_FITTED);
		if (res[(size_t)it.frame].status == SG_MATCH_OK)
			sgm_fwhm_average(stars.data() + (size_t)it.frame * max_stars, it.n, &res[(size_t)it.frame].fwhmx, &res[(size_t)it.frame].fwhmy);
	}
	clock_gettime(CLOCK_MONOTONIC, &t1);
	printf("time %.6f %zu\n", (t1.tv_sec - t0.tv_sec) * 1e3 + (t1.tv_nsec - t0.tv_nsec) * 1e-6, pl.items.size());
	for (int f = 0; f < nframes; f++) {
		const sg_starmatch_result &o = res[(size_t)f];
		printf("frame %d %d %d %d %d %d %d %d %d %d", o.status, o.nbpoints, o.nbright, o.scale_retry, o.nwinners, o.npairs, o.nr_recalc,
				o.inliers, o.ransac_iters, o.lm_iters);
		for (int k = 0; k < 6; k++)
			printf(" %a", o.trans0[k]);
		for (int k = 0; k < 6; k++)
			printf(" %a", o.trans[k]);
		printf(" %a %a %a", o.sig, o.sx, o.sy);
		for (int k = 0; k < 9; k++)
			printf(" %a", o.hom[k]);
		printf(" %a %a %a %a", (double)o.fwhmx, (double)o.fwhmy, o.shiftx, o.shifty);
		const int32_t *p = pairs.data() + (size_t)f * 2 * MAX_STARS_FITTED;
		for (int k = 0; k < 2 * MAX_STARS_FITTED && p[k] >= 0; k++)
			printf(" %d", p[k]);
		printf("\n");
	}
	std::vector<double> hom((size_t)nframes * 9);
	std::vector<int> action((size_t)nframes), slot((size_t)nframes);
	int total = -1;
	const int wr = sgm_warp_plan(res.data(), nframes, hom.data(), action.data(), slot.data(), &total);
	printf("warp %d %d", wr, total);
	for (int f = 0; f < nframes; f++)
		printf(" %d %d", action[(size_t)f], slot[(size_t)f]);
	printf("\n");
	return 0;
}
'''


def build(tmp_path, extra=(), opt="-O1"):
    src = tmp_path / "starmatch_check.cpp"
    src.write_text(PROGRAM)
    exe = tmp_path / "starmatch_check"
    r = subprocess.run(["g++", opt, "-std=c++17", "-ffp-contract=off", "-fno-fast-math", *extra, "-I", INC, str(src),
                        "-o", str(exe), "-lm"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    return exe


def star_arrays(lists, fwhm=None, max_stars=None):
    """(nstars [N] int32, stars [N][max_stars] STAR_DTYPE) as sg_findstar_fit would return the lists"""
    n = len(lists)
    ms = max_stars or max(max(len(L) for L in lists), 1)
    nstars = np.array([len(L) for L in lists], dtype=np.int32)
    stars = np.zeros((n, ms), dtype=STAR_DTYPE)
    for f, L in enumerate(lists):
        L = np.asarray(L, dtype=np.float64).reshape(-1, 3)
        stars["xpos"][f, :len(L)], stars["ypos"][f, :len(L)], stars["mag"][f, :len(L)] = L[:, 0], L[:, 1], L[:, 2]
        if fwhm is not None:
            stars["fwhmx"][f, :len(L)], stars["fwhmy"][f, :len(L)] = fwhm[f][:, 0], fwhm[f][:, 1]
    return nstars, stars


def write_input(path, nstars, stars, ref_image, included=None, nframes=None, max_stars=None):
    n = len(nstars) if nframes is None else nframes
    ms = stars.shape[1] if max_stars is None else max_stars
    blob = [struct.pack("<4i", n, ms, ref_image, 0 if included is None else 1)]
    if included is not None:
        blob.append(np.asarray(included, dtype=np.uint8).tobytes())
    blob.append(np.asarray(nstars, dtype=np.int32).tobytes())
    blob.append(np.ascontiguousarray(stars, dtype=STAR_DTYPE).tobytes())
    path.write_bytes(b"".join(blob))


def parse(stdout):
    """dict(plan = (rc, lds_bytes, grid, nmax, message), ms, frames = [result dicts], warp = (rc, total, action, slot))"""
    out = dict(frames=[], plan=None, warp=None, ms=None)
    for line in stdout.strip().split("\n"):
        t = line.split()
        if t[0] == "plan":
            out["plan"] = (int(t[1]), int(t[2]), int(t[3]), int(t[4]), " ".join(t[5:]))
        elif t[0] == "time":
            out["ms"] = (float(t[1]), int(t[2]))
        elif t[0] == "frame":
            ints = [int(v) for v in t[1:11]]
            fp = [float.fromhex(v) for v in t[11:39]]
            pr = [int(v) for v in t[39:]]
            o = dict(zip(sr.INT_FIELDS, ints))
            o.update(trans0=fp[0:6], trans=fp[6:12], sig=fp[12], sx=fp[13], sy=fp[14], hom=fp[15:24], fwhmx=np.float32(fp[24]),
                     fwhmy=np.float32(fp[25]), shiftx=fp[26], shifty=fp[27], pairs=(pr[0::2], pr[1::2]))
            out["frames"].append(o)
        elif t[0] == "warp":
            v = [int(e) for e in t[1:]]
            out["warp"] = (v[0], v[1], v[2::2], v[3::2])
    return out


def run(exe, tmp_path, nstars, stars, ref_image, included=None, **kw):
    path = tmp_path / "case.bin"
    write_input(path, nstars, stars, ref_image, included, **kw)
    r = subprocess.run([str(exe), str(path)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    return parse(r.stdout)


def compare(got, want, stable, where):
    """the rule both tests hold a result to: every integer field and the pairs exact; trans0, trans, sig, sx, sy,
    hom within TOL (denominator max(|v|, 1)) where the frame is branch-stable; fwhm and the shifts exact / TOL"""
    for k in sr.INT_FIELDS:
        assert int(got[k]) == int(want[k]), (where, k, int(got[k]), int(want[k]))
    assert [list(map(int, p)) for p in got["pairs"]] == [list(map(int, p)) for p in want["pairs"]], (where, "pairs")
    assert np.float32(got["fwhmx"]) == np.float32(want["fwhmx"]) and np.float32(got["fwhmy"]) == np.float32(want["fwhmy"]), (where, "fwhm")
    worst = 0.0
    for k in sr.FP_FIELDS + ("shiftx", "shifty"):
        g, w = np.atleast_1d(np.asarray(got[k], dtype=np.float64)), np.atleast_1d(np.asarray(want[k], dtype=np.float64))
        rel = float((np.abs(g - w) / np.maximum(np.abs(w), 1.0)).max())
        worst = max(worst, rel)
        if stable:
            assert rel <= sr.TOL, (where, k, rel, sr.TOL)
    return worst
