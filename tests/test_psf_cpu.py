"""The per-box part of peaker without a GPU: tests/psf_ref.py (the numpy restatement) against hand-derived
start values, finite differences and scipy's MINPACK, and siril-0.9_amd/csrc/sg_psf.h (what the kernel
calls) built into a stand-alone host program, plainly and under AddressSanitizer + UBSan, fed the same
boxes.  It also holds the conditions tests/test_gpu_starfit.py relies on: for every case it uses, the
unstable boxes, the stable accepted stars and the measured spread behind TOL."""
import os
import struct
import subprocess

import numpy as np
import pytest

import findstar_ref as fsr
import psf_ref as pr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INC = os.path.join(ROOT, "siril-0.9_amd", "csrc")

PROGRAM = r'''
#include <stdio.h>
#include <stdlib.h>
#include <stdint.h>
#include <vector>
#include "sg_psf.h"

/* input: int32 count, then per box int32 r, cx, cy, double bg, norm, scale_x, scale_y, roundness,
 * uint16 box[4 r r] (heap, exactly sized: the sanitizer sees an index past either end) */
int main(int argc, char **argv) {
	if (argc < 2)
		return 2;
	FILE *fi = fopen(argv[1], "rb");
	if (!fi)
		return 2;
	int32_t count;
	if (fread(&count, 4, 1, fi) != 1)
		return 2;
	for (int n = 0; n < count; n++) {
		int32_t h[3];
		double d[5];
		if (fread(h, 4, 3, fi) != 3 || fread(d, 8, 5, fi) != 5)
			return 2;
		std::vector<uint16_t> box((size_t)4 * h[0] * h[0]);
		if (fread(box.data(), 2, box.size(), fi) != box.size())
			return 2;
		double init[6];
		SgPsfFit o;
		sg_psf_fit_box(box.data(), h[0], d[0], h[1], h[2], d[1], d[2], d[3], d[4], init, o);
		printf("%d %d %d", o.status, o.failed_test, o.iters);
		for (int k = 0; k < 6; k++)
			printf(" %a", init[k]);
		printf(" %a %a %a %a %a %a %a %a %a %a %a %a\n", o.B, o.A, o.x0, o.y0, o.sx, o.sy, o.fwhmx, o.fwhmy, o.mag,
				o.rmse, o.xpos, o.ypos);
	}
	fclose(fi);
	return 0;
}
'''

SAN = ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan"]


def _build(tmp_path, extra, opt="-O1"):
    src = tmp_path / "psf_check.cpp"
    src.write_text(PROGRAM)
    exe = tmp_path / "psf_check"
    r = subprocess.run(["g++", opt, "-std=c++17", "-ffp-contract=off", "-fno-fast-math", *extra, "-I", INC, str(src),
                        "-o", str(exe), "-lm"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    return exe


def _run_boxes(exe, tmp_path, items):
    """items: (box [2r][2r] u16, bg, cx, cy, norm, scales, roundness) -> one dict per box"""
    blob = [struct.pack("<i", len(items))]
    for box, bg, cx, cy, norm, scales, roundness in items:
        box = np.ascontiguousarray(box, dtype=np.uint16)
        blob.append(struct.pack("<3i5d", box.shape[0] // 2, cx, cy, bg, norm, scales[0], scales[1], roundness))
        blob.append(box.tobytes())
    path = tmp_path / "boxes.bin"
    path.write_bytes(b"".join(blob))
    r = subprocess.run([str(exe), str(path)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    out = []
    for line in r.stdout.strip().split("\n"):
        t = line.split()
        vals = [float.fromhex(v) if "x" in v else float(v) for v in t[3:]]
        out.append(dict(status=int(t[0]), failed_test=int(t[1]), iters=int(t[2]), init=np.array(vals[:6]),
                        **dict(zip(pr.FIELDS, vals[6:]))))
    assert len(out) == len(items)
    return out


# ------------------------------------------------------------------ start values

def _rule_median(z, x, y):
    """the issue's statement of getMedian3x3: the mean of the 3rd and 4th smallest of 8 neighbours, the
    2nd smallest of 5, the smallest of 3, truncated"""
    h, w = z.shape
    nb = sorted(int(z[j, i]) for j in range(y - 1, y + 2) for i in range(x - 1, x + 2)
                if 0 <= j < h and 0 <= i < w and (i, j) != (x, y))
    if len(nb) == 8:
        return (nb[2] + nb[3]) // 2
    return nb[1] if len(nb) == 5 else nb[0]


def test_median_literal_equals_the_rule():
    rng = np.random.default_rng(1)
    for n2 in (2, 4, 6):
        z = rng.integers(0, 65536, size=(n2, n2)).astype(np.float64)
        z[rng.random((n2, n2)) < 0.2] = 0          # zeros sort among the padding
        for y in range(n2):
            for x in range(n2):
                assert pr.median3x3_literal(z, x, y) == _rule_median(z, x, y)


def test_start_values_by_hand():
    # a corner hot pixel: every filtered value is 100, the first maximum is (0, 0); the walks run on
    # the unfiltered box, move one step down / right and give S = (size_t)(1 / 4 / ln 2) = 0
    z = np.full((4, 4), 100, dtype=np.uint16)
    z[0, 0] = 5000
    assert pr.init_literal(z, 100.0).tolist() == [100.0, 100.0, 1.5, 1.5, 0.0, 0.0]
    # an edge hot pixel (row 0, column 2): filtered away as well; the maximum stays at (0, 0), whose
    # value equals bg: no walk moves
    z = np.full((4, 4), 100, dtype=np.uint16)
    z[0, 2] = 5000
    assert pr.init_literal(z, 100.0).tolist() == [100.0, 100.0, 1.0, 1.0, 0.0, 0.0]
    # a flat box above bg: the walks reach the border (3 - 0 = 3, S = (size_t)(9 / 4 / ln 2) = 3)
    z = np.full((4, 4), 1000, dtype=np.uint16)
    assert pr.init_literal(z, 0.0).tolist() == [0.0, 1000.0, 2.5, 2.5, 3.0, 3.0]
    # an interior hot pixel beside a broad star: the maximum is the star's, not the hot pixel's
    yy, xx = np.mgrid[0:10, 0:10]
    star = np.rint(200 + 8000 * np.exp(-((xx - 5) ** 2 + (yy - 4) ** 2) / 8.0)).astype(np.uint16)
    star[2, 7] = 60000
    init = pr.init_literal(star, 200.0)
    m = pr.remove_hot_pixels(star.astype(np.float64))
    assert m[2, 7] < 8000 and init[1] == m[4, 5] == m.max() and init[1] < 8200
    # half maximum 4000 above bg: rows 4 +- 3 pass 8000 exp(-9/8) = 2597 < 4100, +- 2 do not
    assert init[2:].tolist() == [(8 + 2 + 2) / 2.0, (7 + 1 + 2) / 2.0, float(int(36 / 4.0 / pr.LN2)), float(int(36 / 4.0 / pr.LN2))]


def test_s_zero_is_nonfinite_and_ends():
    z = np.full((6, 6), 100, dtype=np.uint16)
    z[0, 0] = 5000
    o = pr.fit(z, 100.0)
    assert o["status"] == pr.FIT_NONFINITE and o["iters"] == 0 and o["init"][4] == 0.0
    assert pr.fit(np.full((2, 2), 7, dtype=np.uint16), 3.0)["status"] == pr.FIT_NOT_ENOUGH_PIXELS


# ------------------------------------------------------------------ model

def test_jacobian_against_finite_differences():
    rng = np.random.default_rng(2)
    z = rng.integers(500, 4000, size=(10, 10)).astype(np.float64)
    x = np.array([800.0, 9000.0, 5.3, 4.6, 7.5, 5.2])
    f, J = pr.model(x, z)
    # the reference's formula, one pixel at a time
    for i, j in ((0, 0), (3, 7), (9, 9)):
        c = np.exp(-(((j + 1) - x[2]) ** 2 / x[4] + ((i + 1) - x[3]) ** 2 / x[5]))
        assert f[10 * i + j] == x[0] + x[1] * c - z[i, j]
    for k in range(6):
        h = 1e-6 * max(abs(x[k]), 1.0)
        xp, xm = x.copy(), x.copy()
        xp[k] += h
        xm[k] -= h
        fd = (pr.model(xp, z)[0] - pr.model(xm, z)[0]) / (xp[k] - xm[k])
        # the model's own columns 4 and 5 are the reference's: d/dS of exp(-d^2 / S) = + c d^2 / S^2
        assert np.abs(fd - J[:, k]).max() <= 1e-6 * max(np.abs(J[:, k]).max(), 1.0), k


def _sample_boxes():
    """the boxes of findstar_ref.STAR_CASES and of two starfit cases: (box, bg, x, y)"""
    out = []
    for i in range(len(fsr.STAR_CASES)):
        img, r = fsr.star_case(i)
        cands, rec, _ = fsr.candidates(img, 1.0, r)
        out += [(b, rec["median"], x, y) for b, (x, y) in zip(fsr.boxes(img, cands, r), cands)]
    for r in (5, 10):
        img, cands, rec, _ = pr.starfit_case(r)
        out += [(b, rec["median"], x, y) for b, (x, y) in zip(fsr.boxes(img, cands, r), cands)]
    return out


def test_restatement_is_a_working_lm():
    """where the delta test was met before the cap, the parameters agree with scipy's MINPACK run to
    1e-12 from the same start, within LSQ_BOUND = 4 x the largest difference measured here"""
    from scipy.optimize import least_squares
    worst, n = 0.0, 0
    for box, bg, _, _ in _sample_boxes():
        o = pr.fit(box, bg)
        if o["status"] not in (pr.FIT_STAR, pr.FIT_NOT_STAR) or not o["trace"] or o["trace"][-1][1] != "delta test":
            continue
        if o["iters"] >= pr.MAX_ITER:
            continue
        z = np.asarray(box).astype(np.float64)
        res = least_squares(lambda x: pr.model(x, z)[0], o["init"], jac=lambda x: pr.model(x, z)[1], method="lm",
                            xtol=1e-12, ftol=1e-12, gtol=1e-12, x_scale="jac")
        assert res.success
        got = np.array([o["B"] * 65535.0, o["A"] * 65535.0, o["x0"], o["y0"], max(o["sx"], o["sy"]), min(o["sx"], o["sy"])])
        want = np.array([res.x[0], res.x[1], res.x[2], res.x[3], max(res.x[4], res.x[5]), min(res.x[4], res.x[5])])
        worst = max(worst, float((np.abs(got - want) / np.maximum(np.abs(want), 1.0)).max()))
        n += 1
    print("converged boxes", n, "largest relative difference", worst, "bound", pr.LSQ_BOUND)
    assert n >= 10
    assert worst <= pr.LSQ_BOUND


# ------------------------------------------------------------------ sg_psf.h on the host

def _check_program(exe, tmp_path):
    items, want = [], []
    for box, bg, x, y in _sample_boxes():
        items.append((box, bg, x, y, 65535.0, (1.0, 1.0), 0.5))
    # the hand-made boxes: S = 0 (not finite, ends), too few pixels, a flat box, norm 255 and scales
    z = np.full((6, 6), 100, dtype=np.uint16)
    z[0, 0] = 5000
    items.append((z, 100.0, 7, 9, 65535.0, (1.0, 1.0), 0.5))
    items.append((np.full((2, 2), 7, dtype=np.uint16), 3.0, 1, 1, 65535.0, (1.0, 1.0), 0.5))
    items.append((np.full((4, 4), 1000, dtype=np.uint16), 0.0, 2, 2, 65535.0, (1.0, 1.0), 0.5))
    items.append((np.zeros((4, 4), dtype=np.uint16), 0.0, 2, 2, 65535.0, (1.0, 1.0), 0.5))
    b0 = items[0]
    items.append((b0[0], b0[1], b0[2], b0[3], 255.0, (1.7, 0.9), 0.8))
    got = _run_boxes(exe, tmp_path, items)
    nfit = 0
    for g, (box, bg, x, y, norm, scales, rnd) in zip(got, items):
        outs = {name: pr.fit(box, bg, name, x, y, norm, scales, rnd) for name in pr.ALL_VARIANTS}
        w = outs["base"]
        assert g["init"].tobytes() == w["init"].tobytes(), (g["init"], w["init"])
        stable, _ = pr.classify(outs, rnd, pr.TOL)
        if not stable:
            assert 0 <= g["status"] <= pr.FIT_NOT_STAR
            continue
        assert (g["status"], g["failed_test"], g["iters"]) == (w["status"], w["failed_test"], w["iters"]), (g, w)
        if w["status"] in (pr.FIT_STAR, pr.FIT_NOT_STAR, pr.FIT_BAD_FWHM):
            nfit += 1
            for k in pr.FIELDS:
                a, b = g[k], float(w[k])
                assert (np.isnan(a) and np.isnan(b)) or a == b or abs(a - b) <= pr.TOL * max(abs(b), 1.0), (k, a, b)
    assert nfit >= 30
    assert got[-5]["status"] == pr.FIT_NONFINITE and got[-4]["status"] == pr.FIT_NOT_ENOUGH_PIXELS


def test_fit_box_program(tmp_path):
    _check_program(_build(tmp_path, []), tmp_path)


def test_fit_box_program_sanitized(tmp_path):
    """the same program under AddressSanitizer + UBSan (host code only, run stand-alone)"""
    probe = tmp_path / "probe.c"
    probe.write_text("int main(void) { return 0; }\n")
    p = subprocess.run(["gcc", *SAN, str(probe), "-o", str(tmp_path / "probe")], capture_output=True, text=True)
    if p.returncode != 0 or subprocess.run([str(tmp_path / "probe")]).returncode != 0:
        pytest.skip("the AddressSanitizer / UBSan runtime is not installed")
    _check_program(_build(tmp_path, SAN, "-O0"), tmp_path)


# ------------------------------------------------------------------ what the GPU tests rely on

@pytest.mark.parametrize("r", sorted(pr.STARFIT_CASES))
def test_gpu_case_conditions(r):
    img, cands, rec, tail = pr.starfit_case(r)
    assert img.shape[0] <= 160 and img.shape[1] <= 160 and len(cands) >= 30
    stable = tail["stable"]
    accepted = [n for n in tail["stars"] if stable[n]]
    print("r", r, "candidates", len(cands), "unstable", int((~stable).sum()), "stable stars", len(accepted),
          "spread", tail["spread"])
    assert (~stable).sum() <= 0.05 * len(cands)
    assert len(accepted) >= 10
    assert tail["spread"] <= pr.TOL / 16
    # the three special stars are among the candidates' boxes
    # the star centred exactly r from the left border is a candidate whose box starts at column 0; at
    # r = 2 the clamped smoothing moves the plane's peak to x = 1, outside the scan rectangle
    assert r == 2 or any(x == r for x, _ in cands), "no candidate exactly r from the border"
    assert (img == 65535).sum() >= 4, "no clipped star"
    assert (img == 60000).sum() >= 1, "no hot pixel"


def test_spread_within_tol():
    """TOL = 16 x the largest spread of any reported field across the variants over the stable boxes
    of all cases; the spread is recomputed here"""
    spread = max(pr.starfit_case(r)[3]["spread"] for r in pr.STARFIT_CASES)
    for kw in (dict(norm=255.0), dict(scales=(1.0, 0.62), roundness=0.7)):
        spread = max(spread, pr.starfit_case(10, **kw)[3]["spread"])
    for plane, r in pr.starfit_extra_frames():
        cands, rec, _ = fsr.candidates(plane, pr.K_SIGMA, r)
        tail = pr.peaker_tail(plane, cands[:64], r, rec["median"], variants=pr.ALL_VARIANTS)
        assert (~tail["stable"]).sum() <= 0.05 * len(cands)
        spread = max(spread, tail["spread"])
    print("spread", spread, "TOL", pr.TOL)
    assert 0 < spread <= pr.TOL / 16
