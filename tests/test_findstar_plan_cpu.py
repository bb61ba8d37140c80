"""The host-only plan of a star-candidate call (siril-0.9_amd/csrc/sg_findstar_plan.hpp), built for the
host and checked without a GPU: the refused arguments and their codes, the wavelet decision at sides
31 and 32, empty scan rectangles, the tile grid and halo around a tile multiple, LDS and scratch
sizes, the WORD conversion of the threshold, and the fused two-pass tile (the functions the kernel
calls per column strip) emulated tile by tile with exactly sized LDS arrays against a plain two-pass
smooth of the whole image, which under AddressSanitizer is the bounds check of the kernel's index
arithmetic."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INC = os.path.join(ROOT, "siril-0.9_amd", "csrc")

PROGRAM = r'''
#include <stdio.h>
#include <stdlib.h>
#include <stdint.h>
#include <string.h>
#include <math.h>
#include <limits>
#include <vector>
#include "sg_findstar_plan.hpp"

static int bad = 0, checks = 0;
#define CHECK(cond) do { checks++; if (!(cond)) { if (bad < 40) printf("FAIL %s:%d: %s\n", __func__, __LINE__, #cond); bad++; } } while (0)

static sg_findstar_desc desc(int W, int H, int C = 1, int layer = 0, int r = 3, double k = 1.0, int maxc = 100) {
	sg_findstar_desc d;
	memset(&d, 0, sizeof d);
	d.width = W;
	d.height = H;
	d.nb_layers = C;
	d.layer = layer;
	d.radius = r;
	d.sigma = k;
	d.max_candidates = maxc;
	return d;
}

static int plan(sg_findstar_desc d, SgFindstarPlan &p) { return sg_findstar_plan(&d, p); }

static sg_findstar_desc with_area(sg_findstar_desc d, int x, int y, int w, int h) {
	d.use_area = 1;
	d.area.x = x;
	d.area.y = y;
	d.area.w = w;
	d.area.h = h;
	return d;
}

static void test_errors(void) {
	SgFindstarPlan p;
	CHECK(sg_findstar_plan(nullptr, p) == SG_ERR_GENERIC);
	CHECK(plan(desc(0, 10), p) == SG_ERR_SIZE && p.err[0]);
	CHECK(plan(desc(10, -1), p) == SG_ERR_SIZE);
	CHECK(plan(desc(10, 10, 0), p) == SG_ERR_SIZE);
	CHECK(plan(desc(65536, 32768), p) == SG_ERR_SIZE);	/* 2^31 pixels */
	CHECK(plan(desc(65536, 32767), p) == SG_OK);
	CHECK(plan(desc(64, 64, 3, 3), p) == SG_ERR_SIZE);
	CHECK(plan(desc(64, 64, 3, -1), p) == SG_ERR_SIZE);
	CHECK(plan(desc(64, 64, 3, 2), p) == SG_OK && p.layer == 2 && p.C == 3);
	CHECK(plan(with_area(desc(64, 64), -1, 0, 10, 10), p) == SG_ERR_SIZE);
	CHECK(plan(with_area(desc(64, 64), 0, 0, 65, 10), p) == SG_ERR_SIZE);
	CHECK(plan(with_area(desc(64, 64), 60, 0, 5, 10), p) == SG_ERR_SIZE);
	CHECK(plan(with_area(desc(64, 64), 0, 60, 10, 5), p) == SG_ERR_SIZE);
	CHECK(plan(with_area(desc(64, 64), 0, 0, 10, -2), p) == SG_ERR_SIZE);
	CHECK(plan(with_area(desc(64, 64), 2147483647, 0, 2147483647, 1), p) == SG_ERR_SIZE);
	CHECK(plan(with_area(desc(64, 64), 59, 54, 5, 10), p) == SG_OK);
	CHECK(plan(desc(64, 64, 1, 0, 0), p) == SG_ERR_GENERIC);
	CHECK(plan(desc(64, 64, 1, 0, -3), p) == SG_ERR_GENERIC);
	CHECK(plan(desc(64, 64, 1, 0, 3, -0.5), p) == SG_ERR_GENERIC);
	CHECK(plan(desc(64, 64, 1, 0, 3, NAN), p) == SG_ERR_GENERIC);
	CHECK(plan(desc(64, 64, 1, 0, 3, INFINITY), p) == SG_ERR_GENERIC);
	CHECK(plan(desc(64, 64, 1, 0, 3, 0.0), p) == SG_OK && p.err[0] == 0);
	CHECK(plan(desc(64, 64, 1, 0, 3, 1.0, -1), p) == SG_ERR_GENERIC);
	CHECK(plan(desc(64, 64, 1, 0, 3, 1.0, 0), p) == SG_OK && p.max_candidates == 0);
	/* the size checks come first: a bad size with a bad radius is a size error */
	CHECK(plan(desc(0, 64, 1, 0, 0), p) == SG_ERR_SIZE);
}

static void test_wavelet_decision(void) {
	SgFindstarPlan p;
	CHECK(plan(desc(31, 64), p) == SG_OK && !p.wavelet);
	CHECK(plan(desc(64, 31), p) == SG_OK && !p.wavelet);
	CHECK(plan(desc(32, 32), p) == SG_OK && p.wavelet);
	CHECK(plan(desc(32, 4096), p) == SG_OK && p.wavelet);
	CHECK(plan(desc(1, 1, 1, 0, 1), p) == SG_OK && !p.wavelet && p.scan_w == 0);
}

static void test_scan_rect(void) {
	SgFindstarPlan p;
	CHECK(plan(desc(48, 40, 1, 0, 5), p) == SG_OK && p.sx0 == 5 && p.sy0 == 5 && p.scan_w == 38 && p.scan_h == 30);
	CHECK(p.box_elems == 100 && p.mask_words == 1);
	CHECK(plan(desc(48, 40, 1, 0, 20), p) == SG_OK && p.scan_w == 0 && p.scan_h == 0 && p.mask_words == 0);	/* 2r == H */
	CHECK(p.mask_bytes == 0 && p.box_elems == 0);
	CHECK(plan(desc(48, 40, 1, 0, 19), p) == SG_OK && p.scan_w == 10 && p.scan_h == 2);
	CHECK(plan(desc(48, 40, 1, 0, 24), p) == SG_OK && p.scan_w == 0);	/* 2r == W */
	CHECK(plan(desc(48, 40, 1, 0, 2147483647), p) == SG_OK && p.scan_w == 0);	/* no overflow */
	CHECK(plan(with_area(desc(130, 96, 1, 0, 3), 7, 11, 41, 33), p) == SG_OK);
	CHECK(p.sx0 == 10 && p.sy0 == 14 && p.scan_w == 35 && p.scan_h == 27 && p.ax1 == 48 && p.ay1 == 44);
	CHECK(plan(with_area(desc(130, 96, 1, 0, 3), 7, 11, 6, 33), p) == SG_OK && p.scan_w == 0);
	CHECK(plan(with_area(desc(130, 96, 1, 0, 3), 7, 11, 0, 0), p) == SG_OK && p.scan_w == 0);
	CHECK(plan(desc(4096, 4096, 1, 0, 10), p) == SG_OK && p.scan_w == 4076 && p.mask_words == 64);
	CHECK(p.mask_bytes == (size_t)4076 * 64 * 8 && p.rows_bytes == 4077 * 4);
	CHECK(plan(desc(200, 31, 1, 0, 1), p) == SG_OK && p.scan_w == 198 && p.mask_words == 4 && p.scan_h == 29);
}

static void test_tiles_and_sizes(void) {
	SgFindstarPlan p;
	CHECK(SGF_TILE_W == 64 && SGF_TILE_H == 32 && SGF_HALO == 6 && SGF_HALO2 == 4);
	CHECK(SGF_P1_ITEMS == 8 * 72 && SGF_P2_ITEMS == 256);	/* strips: 5 rows of pass 1, 8 rows of pass 2 */
	const int w[3] = {63, 64, 65}, tx[3] = {1, 1, 2};
	for (int i = 0; i < 3; i++)
		CHECK(plan(desc(w[i], 40), p) == SG_OK && p.tiles_x == tx[i] && p.tiles_y == 2 && p.halo == 6);
	const int h[3] = {63, 64, 65}, ty[3] = {2, 2, 3};
	for (int i = 0; i < 3; i++)
		CHECK(plan(desc(40, h[i]), p) == SG_OK && p.tiles_y == ty[i] && p.tiles_x == 1);
	CHECK(plan(desc(4096, 4096), p) == SG_OK && p.tiles_x == 64 && p.tiles_y == 128);
	CHECK(p.in_w == 76 && p.in_h == 44 && p.mid_w == 72 && p.mid_h == 40);
	CHECK(p.lds_bytes == 76 * 44 * 2 + 72 * 40 * 4 && p.lds_bytes == 18208);	/* 8 workgroups in 160 KiB */
	CHECK(p.hist_bytes == 262144 && p.stat_bytes == 32 && p.plane_bytes == (size_t)4096 * 4096 * 2);
	CHECK(sgf_chunk_frames(p, 64, 0) == 32 && sgf_chunk_frames(p, 64, 1) == 64 && sgf_chunk_frames(p, 1000, 1) == 256);
	CHECK(sgf_chunk_frames(p, 5, 0) == 5);
	CHECK(plan(desc(65536, 32767), p) == SG_OK && sgf_chunk_frames(p, 8, 0) == 1);
}

static void test_threshold(void) {
	int w;
	CHECK(sgf_to_word(65535.9) == 65535 && sgf_to_word(65536.0) == 0 && sgf_to_word(65537.5) == 1);
	CHECK(sgf_to_word(2147483647.5) == 0xFFFF && sgf_to_word(2147483648.0) == 0 && sgf_to_word(NAN) == 0);
	CHECK(sgf_to_word(1e300) == 0 && sgf_to_word(-1.5) == 0xFFFF);
	CHECK(sgf_threshold(802.0, 2261.7, 1.0, &w) == 3063 && !w);
	CHECK(sgf_threshold(802.0, 2261.7, 0.5, &w) == 802 + 1130 && !w);	/* k * (WORD)sigma, truncated at the end */
	CHECK(sgf_threshold(802.0, 2261.7, 100.0, &w) == (uint16_t)(802 + 226100) && w);
	CHECK(sgf_threshold(0.0, 30000.0, 1e9, &w) == 0 && w);
	CHECK(sgf_threshold(65535.0, 0.0, 3.0, &w) == 65535 && !w);
	CHECK(sgf_sums_exact(((uint64_t)1 << 53) - 1) && !sgf_sums_exact((uint64_t)1 << 53));
	/* sigma from the sums equals the sequential loop while the sums are exact */
	std::vector<uint16_t> a(5000);
	uint64_t n = 0, s = 0, s2 = 0;
	for (size_t i = 0; i < a.size(); i++) {
		a[i] = (uint16_t)((i * 2654435761u) >> 13);
		if (i % 7 == 0)
			a[i] = 0;
		if (a[i]) {
			n++;
			s += a[i];
			s2 += (uint64_t)a[i] * a[i];
		}
	}
	const double x = sgf_sigma_sums(n, s, s2), y = sgf_sigma_seq(a.data(), (int64_t)a.size());
	CHECK(memcmp(&x, &y, sizeof x) == 0 && x > 0);
	CHECK(sgf_sigma_sums(1, 777, 777 * 777) == 0.0 && sgf_sigma_sums(0, 0, 0) == 0.0);
	uint16_t one[4] = {0, 0, 9, 0};
	CHECK(sgf_sigma_seq(one, 4) == 0.0);
}

/* pave_2d_bspline_smooth over a whole image, plainly */
static std::vector<float> smooth(const std::vector<float> &in, int W, int H, int step) {
	std::vector<float> out((size_t)W * H);
	for (int i = 0; i < H; i++)
		for (int j = 0; j < W; j++) {
			const float *r3 = &in[(size_t)sgf_clamp(i - 2 * step, H) * W], *r1 = &in[(size_t)sgf_clamp(i - step, H) * W];
			const float *r0 = &in[(size_t)i * W];
			const float *r2 = &in[(size_t)sgf_clamp(i + step, H) * W], *r4 = &in[(size_t)sgf_clamp(i + 2 * step, H) * W];
			out[(size_t)i * W + j] = sgf_bspline(r3, r1, r0, r2, r4, sgf_clamp(j - 2 * step, W), sgf_clamp(j - step, W), j,
					sgf_clamp(j + step, W), sgf_clamp(j + 2 * step, W));
		}
	return out;
}

/* the kernel's tile, with LDS arrays of exactly the kernel's sizes (heap: the sanitizer sees an
 * index one past either end) */
static void test_tiles_equal_whole_image(void) {
	const int shapes[][2] = {{32, 32}, {33, 32}, {32, 33}, {70, 37}, {130, 70}, {63, 64}, {65, 31 + 2}, {200, 40}};
	for (auto &sh : shapes) {
		const int W = sh[0], H = sh[1];
		std::vector<uint16_t> img((size_t)W * H);
		uint32_t x = 12345u + W * 131 + H;
		for (auto &v : img) {
			x = x * 1664525u + 1013904223u;
			v = (uint16_t)(x >> 16);
		}
		std::vector<float> f(img.begin(), img.end());
		const std::vector<float> want = smooth(smooth(f, W, H, 1), W, H, 2);
		SgFindstarPlan p;
		CHECK(plan(desc(W, H), p) == SG_OK && p.wavelet);
		std::vector<float> got((size_t)W * H, -1.f);
		for (int ty = 0; ty < p.tiles_y; ty++)
			for (int tx = 0; tx < p.tiles_x; tx++) {
				std::vector<uint16_t> s_in((size_t)p.in_w * p.in_h);
				std::vector<float> s_mid((size_t)p.mid_w * p.mid_h, std::numeric_limits<float>::quiet_NaN());
				const int tx0 = tx * SGF_TILE_W, ty0 = ty * SGF_TILE_H;
				for (int idx = 0; idx < p.in_w * p.in_h; idx++)
					s_in[idx] = sgf_tile_load(idx, img.data(), W, H, tx0, ty0);
				for (int item = 0; item < SGF_P1_ITEMS; item++)
					sgf_tile_pass1(item, s_in.data(), s_mid.data(), W, H, tx0, ty0);
				for (int item = 0; item < SGF_P2_ITEMS; item++) {
					int gy0, gx;
					float v[SGF_P2_ROWS];
					const int n = sgf_tile_pass2(item, s_mid.data(), W, H, tx0, ty0, &gy0, &gx, v);
					for (int u = 0; u < n; u++) {
						CHECK(gy0 + u < H && gx < W && got[(size_t)(gy0 + u) * W + gx] == -1.f);	/* every pixel once */
						got[(size_t)(gy0 + u) * W + gx] = v[u];
					}
				}
			}
		CHECK(memcmp(got.data(), want.data(), sizeof(float) * got.size()) == 0);
	}
}

int main(void) {
	test_errors();
	test_wavelet_decision();
	test_scan_rect();
	test_tiles_and_sizes();
	test_threshold();
	test_tiles_equal_whole_image();
	printf("checks=%d bad=%d\n", checks, bad);
	return bad ? 1 : 0;
}
'''


def _build(tmp_path, extra, opt="-O1"):
    src = tmp_path / "findstar_plan_check.cpp"
    src.write_text(PROGRAM)
    exe = tmp_path / "findstar_plan_check"
    r = subprocess.run(["g++", opt, "-std=c++17", "-ffp-contract=off", "-fno-fast-math", *extra,
                        "-I", INC, str(src), "-o", str(exe), "-lm"], capture_output=True, text=True)
    return exe, r


def _run(exe):
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    assert " bad=0" in r.stdout and "checks=" in r.stdout, r.stdout[-2000:]


def test_findstar_plan_known_answers(tmp_path):
    exe, r = _build(tmp_path, [])
    assert r.returncode == 0, r.stderr[-4000:]
    _run(exe)


def test_findstar_plan_sanitized(tmp_path):
    """the same program under AddressSanitizer + UBSan (host code only, run stand-alone)"""
    # the runtimes are linked statically: the program then runs whatever else the loader brings in
    san = ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan"]
    probe = tmp_path / "probe.c"
    probe.write_text("int main(void) { return 0; }\n")
    p = subprocess.run(["gcc", *san, str(probe), "-o", str(tmp_path / "probe")], capture_output=True, text=True)
    if p.returncode != 0 or subprocess.run([str(tmp_path / "probe")]).returncode != 0:
        pytest.skip("the AddressSanitizer / UBSan runtime is not installed")
    exe, r = _build(tmp_path, san, "-O0")
    assert r.returncode == 0, r.stderr[-4000:]
    _run(exe)
