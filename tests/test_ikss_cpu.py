"""The IKSS solver the device runs (siril-0.9_amd/csrc/sg_ikss.h: rank lookups on the prefix
table, two-sided MAD merge, run-length BWMV sums, clipping searches), built for the host and
compared bit for bit with the oracle's sort-based restatement of statistics()
(oracle/or_statistics.c) on random sample sets.  The program builds the 65536-bin histogram
and the exclusive prefix as k_ikss_prefix defines them; what the GPU adds to this (histogram
kernels, frame strides, passes) is tests/test_gpu_stats.py's part."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INC = os.path.join(ROOT, "siril-0.9_amd", "csrc")
ORC = os.path.join(ROOT, "oracle")
ORC_CFLAGS = ["-O2", "-fopenmp", "-fPIC", "-ffp-contract=off", "-fno-fast-math"]    # oracle/Makefile
NSETS = 1800
NSETS_SANITIZED = 300

PROGRAM = r'''
#include <stdio.h>
#include <stdlib.h>
#include <stdint.h>
#include <string.h>
#include <math.h>
#include <vector>
#include "sg_ikss.h"
extern "C" int or_statistics_ikss(const uint16_t *frame, int C, int H, int W, double *location, double *scale);

static uint64_t s = 88172645463325252ull;
static uint64_t rnd(void) { s ^= s << 13; s ^= s >> 7; s ^= s << 17; return s; }
static double uni(void) { return (double)(rnd() >> 11) / 9007199254740992.0; }	/* [0, 1) */
static double gauss(void) { return sqrt(-2.0 * log(1.0 - uni())) * cos(6.283185307179586 * uni()); }
static uint16_t u16(double v) { return v < 0 ? 0 : v > 65535 ? 65535 : (uint16_t)v; }

enum { NF = 3, F = 1 };	/* the table is frame-minor: the set under test is column 1 of 3 */

/* location / scale / rc of layer 0 of d[C][n] through the solver; 1 when they equal the oracle's */
static int check(const std::vector<uint16_t> &d, int C, int n, int t, int fam) {
	static std::vector<uint32_t> P((size_t)(SG_IK_BINS + 1) * NF);
	std::vector<uint32_t> h(SG_IK_BINS, 0);
	uint32_t maxi = 0;
	for (int i = 0; i < n; i++)
		if (d[i])
			h[d[i]]++;	/* zeros are null pixels: not counted */
	for (size_t i = 0; i < d.size(); i++)
		maxi = d[i] > maxi ? d[i] : maxi;	/* over all layers */
	uint32_t run = 0;
	for (int x = 0; x <= SG_IK_BINS; x++) {	/* exclusive prefix, row SG_IK_BINS = total */
		P[(size_t)x * NF + 0] = (uint32_t)rnd();
		P[(size_t)x * NF + F] = run;
		P[(size_t)x * NF + 2] = (uint32_t)rnd();
		if (x < SG_IK_BINS)
			run += h[x];
	}
	double gl = -1, gs = -1, ol = -1, os = -1;
	const int grc = sg_ikss_frame(P.data(), NF, F, maxi, &gl, &gs);
	const int orc = or_statistics_ikss(d.data(), C, 1, n, &ol, &os);
	if (grc != orc || (orc == 0 && (memcmp(&gl, &ol, 8) != 0 || memcmp(&gs, &os, 8) != 0))) {
		printf("set %d family %d n=%d C=%d: rc %d %d location %.17g %.17g scale %.17g %.17g\n", t, fam, n, C, grc, orc,
				gl, ol, gs, os);
		return 0;
	}
	return 1;
}

int main(int argc, char **argv) {
	const int nsets = argc > 1 ? atoi(argv[1]) : 1500;
	int bad = 0;
	for (int t = 0; t < nsets; t++) {
		int fam = t % 8, n = 7 + (int)(rnd() % 20000), C = 1;
		if (t % 50 == 49)
			n = 1 + (int)(rnd() % 6);
		else if (t % 30 == 7) {
			fam = 8;	/* few distinct values, huge counts: sg_add_repeat's long runs */
			n = 1000 + (int)(rnd() % 199001);
		}
		std::vector<uint16_t> d(n);
		const double mean = 200 + uni() * 65000, sigma = 0.3 + uni() * uni() * 3000;
		switch (fam) {
		case 0:	/* gaussian at random mean and sigma (clamped: mass piles up at 0 = null and at 65535) */
			for (int i = 0; i < n; i++)
				d[i] = u16(mean + sigma * gauss());
			break;
		case 1: {	/* 8-bit data: norm 255 ... */
			const double m8 = 20 + uni() * 215, s8 = 0.3 + uni() * 40;
			for (int i = 0; i < n; i++) {
				const double v = m8 + s8 * gauss();
				d[i] = v < 0 ? 0 : v > 255 ? 255 : (uint16_t)v;
			}
			if (t % 16 == 9) {	/* ... unless another layer holds a larger value */
				C = 2;
				d.resize(2 * (size_t)n, 7);
				d[n + rnd() % n] = 256 + (uint16_t)(rnd() % 3);
			}
			break;
		}
		case 2: {	/* tight gaussian + 10 % uniform outliers: clipping advances both ends */
			const double m = 3000 + uni() * 50000, sg = 2 + uni() * 60;
			for (int i = 0; i < n; i++)
				d[i] = rnd() % 10 == 0 ? (uint16_t)rnd() : u16(m + sg * gauss());
			break;
		}
		case 3: {	/* mostly one value with a few neighbours: MAD 0 */
			const uint16_t v = (uint16_t)(2 + rnd() % 65532);
			const int k = (int)(rnd() % 8), w = 1 + (int)(rnd() % 3);
			for (int i = 0; i < n; i++)
				d[i] = v;
			for (int i = 0; i < k && i < n / 2 - 1; i++)
				d[rnd() % n] = (uint16_t)(v - w + (int)(rnd() % (2 * w + 1)));
			break;
		}
		case 4:	/* {0..3} u {65535} */
			for (int i = 0; i < n; i++)
				d[i] = rnd() % 5 == 4 ? 65535 : (uint16_t)(rnd() % 4);
			break;
		case 5: {	/* bimodal */
			const double m2 = 200 + uni() * 65000, s2 = 0.3 + uni() * 500, p = 0.05 + 0.9 * uni();
			for (int i = 0; i < n; i++)
				d[i] = uni() < p ? u16(mean + sigma * gauss()) : u16(m2 + s2 * gauss());
			break;
		}
		case 6: {	/* crowded against 65535 */
			const double sc = 1 + uni() * 400;
			for (int i = 0; i < n; i++)
				d[i] = u16(65535.9 - fabs(sc * gauss()));
			break;
		}
		case 7: {	/* heavy tails (Cauchy) */
			const double g = 1 + uni() * 300;
			for (int i = 0; i < n; i++)
				d[i] = u16(mean + g * tan(3.141592653589793 * (uni() - 0.5)));
			break;
		}
		default: {
			const double sg = 0.4 + uni() * 4;
			for (int i = 0; i < n; i++)
				d[i] = u16(mean + sg * gauss());
		}
		}
		bad += !check(d, C, n, t, fam);
	}
	/* an all-zero set: rc -1 on both sides */
	{
		std::vector<uint16_t> z(100, 0);
		double l, sc;
		bad += !check(z, 1, 100, -1, -1);
		if (or_statistics_ikss(z.data(), 1, 1, 100, &l, &sc) != -1) {
			printf("all-zero set: rc is not -1\n");
			bad++;
		}
	}
	printf("sets=%d bad=%d\n", nsets + 1, bad);
	return bad != 0;
}
'''


def _build(tmp_path, extra):
    src = tmp_path / "ikss_fuzz.cpp"
    src.write_text(PROGRAM)
    obj = tmp_path / "or_statistics.o"
    exe = tmp_path / "ikss_fuzz"
    r = subprocess.run(["gcc", *ORC_CFLAGS, *extra, "-I", ORC, "-c", os.path.join(ORC, "or_statistics.c"), "-o", str(obj)],
                       capture_output=True, text=True)
    if r.returncode == 0:
        r = subprocess.run(["g++", "-O2", "-ffp-contract=off", "-fno-fast-math", *extra, "-I", INC, str(src), str(obj),
                            "-o", str(exe), "-lm"], capture_output=True, text=True)
    return exe, r


def test_ikss_solver_matches_oracle(tmp_path):
    exe, r = _build(tmp_path, [])
    assert r.returncode == 0, r.stderr
    r = subprocess.run([str(exe), str(NSETS)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-2000:]
    assert "sets=%d bad=0" % (NSETS + 1) in r.stdout


def test_ikss_solver_sanitized(tmp_path):
    """the same program under AddressSanitizer + UBSan (host code only, run stand-alone)"""
    # the runtimes are linked statically: the program then runs whatever else the loader brings in
    san = ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan"]
    probe = tmp_path / "probe.c"
    probe.write_text("int main(void) { return 0; }\n")
    p = subprocess.run(["gcc", *san, str(probe), "-o", str(tmp_path / "probe")], capture_output=True, text=True)
    if p.returncode != 0 or subprocess.run([str(tmp_path / "probe")]).returncode != 0:
        pytest.skip("the AddressSanitizer / UBSan runtime is not installed")
    exe, r = _build(tmp_path, san)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([str(exe), str(NSETS_SANITIZED)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    assert "sets=%d bad=0" % (NSETS_SANITIZED + 1) in r.stdout
