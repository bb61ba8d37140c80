"""Automatic cosmetic correction without a GPU: the two numpy forms of
tests/cosme_ref.py against each other on every case the GPU tests run, the statistics against
prepro_ref.hist_median and a direct absdev, the scan-order dependence pinned (a one-pass
implementation fails), and siril-0.9_amd/csrc/sg_cosme.h built as a stand-alone host program that
runs whole small frames tile by tile with exactly sized tile arrays, plainly and under
AddressSanitizer + UBSan, equal to the literal form bit for bit."""
import os
import struct
import subprocess

import numpy as np
import pytest

import cosme_cases as cc
import cosme_ref as cr
import prepro_ref as pr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INC = os.path.join(ROOT, "siril-0.9_amd", "csrc")
SAN = ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan"]


# ------------------------------------------------------------------ 1. literal == rule

@pytest.mark.parametrize("name", sorted(cc.CASES))
def test_rule_equals_literal(name):
    case = cc.CASES[name]
    for f, frame in enumerate(cc.frames_of(name)):
        want, wres = cc.literal_of(name)[f]
        got, gres, _ = cr.autodetect_rule(frame, case["sig"], case["amount"], case["is_cfa"])
        assert np.array_equal(got, want), (name, f, int((got != want).sum()))
        assert gres == wres, (name, f, gres, wres)


def test_cases_exercise_both_tests_and_chains():
    """the case list is not vacuous: hot and cold hits, corrections that differ from one pass"""
    hot = sum(r["ihot"] for n in cc.CASES for _, r in cc.literal_of(n))
    cold = sum(r["icold"] for n in cc.CASES for _, r in cc.literal_of(n))
    assert hot > 100 and cold > 100
    for name in ("chain_h", "chain_v", "chain_d", "chain_comb", "chain_h_cfa", "chain_comb_cfa"):
        frame = cc.frames_of(name)[0]
        case = cc.CASES[name]
        _, _, infos = cr.autodetect_rule(frame, case["sig"], case["amount"], case["is_cfa"])
        assert infos[0]["rounds"] >= (60 if not case["is_cfa"] else 30), (name, infos[0]["rounds"])


# ------------------------------------------------------------------ 2. the statistics

@pytest.mark.parametrize("seed", [0, 1, 2])
def test_statistics_from_the_histogram(seed):
    rng = np.random.default_rng(seed)
    p = cr.dense_plane(37, 53, seed)
    p[rng.random(p.shape) < 0.1] = 0
    p[rng.random(p.shape) < 0.05] = 65535
    ngood, bkg, avg = cr.statistics_hist(p)
    g = p.reshape(-1)
    nz = g[g != 0]
    assert ngood == nz.size and bkg == pr.hist_median(g, nz.size)
    direct = 0.0
    for v in nz.tolist():                      # gsl_stats_ushort_absdev_m's loop
        direct += abs(v - bkg)
    assert avg == direct / nz.size
    assert cr.statistics(p) == (ngood, bkg, avg)


def test_statistics_edge_planes():
    assert cr.statistics_hist(np.zeros((4, 5), np.uint16)) is None and cr.statistics(np.zeros((4, 5), np.uint16)) is None
    full = np.full((4, 5), 65535, np.uint16)
    assert cr.statistics_hist(full) == (20, 0.0, 65535.0) == cr.statistics(full)
    one = np.zeros((4, 5), np.uint16)
    one[2, 3] = 7
    assert cr.statistics_hist(one) == (1, 7.0, 0.0) == cr.statistics(one)


# ------------------------------------------------------------------ 3. the dependence, pinned

# (is_cfa): corrected serially (cold, hot), corrected by one pass over the original, pixels where the
# two outputs differ, rounds until the fixed point.  From autodetect_literal on cosme_ref.dependence_case().
PINNED = {False: ((44, 74), (44, 28), 69, 39), True: ((44, 82), (44, 43), 75, 19)}


@pytest.mark.parametrize("is_cfa", [False, True])
def test_dependence_pinned(is_cfa):
    p = cr.dependence_case()[None]
    serial, sres = cr.autodetect_literal(p, (3.0, 1.0), 1.0, is_cfa)
    got, gres, infos = cr.autodetect_rule(p, (3.0, 1.0), 1.0, is_cfa)
    want_serial, want_one, want_diff, want_rounds = PINNED[is_cfa]
    assert (sres["icold"], sres["ihot"]) == want_serial
    assert np.array_equal(got, serial) and gres == sres
    assert infos[0]["one_pass"] == want_one
    assert int((infos[0]["one_pass_plane"] != serial[0]).sum()) == want_diff
    assert infos[0]["rounds"] == want_rounds
    # a bounded number of rounds is not enough: the chains are as long as the run
    short = cr.autodetect_layer_rule(p[0], (3.0, 1.0), 1.0, is_cfa, max_rounds=4)
    assert not np.array_equal(short[0], serial[0])


# ------------------------------------------------------------------ 4. sg_cosme.h as a host program

PROGRAM = r"""
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
#include "sg_cosme.h"

struct Head { int W, H, C, is_cfa; double sig0, sig1, amount; };
struct Res { int status, failed_layer; long long icold, ihot; double bkg[3], avg_dev[3]; long long rounds, medians; };

int main(int argc, char **argv) {
	if (argc != 3)
		return 2;
	FILE *fi = fopen(argv[1], "rb");
	Head h;
	if (!fi || fread(&h, sizeof h, 1, fi) != 1)
		return 3;
	const int W = h.W, H = h.H;
	const size_t npix = (size_t)W * H;
	std::vector<uint16_t> frame(npix * h.C);
	if (fread(frame.data(), 2, frame.size(), fi) != frame.size())
		return 4;
	fclose(fi);
	Res res;
	memset(&res, 0, sizeof res);
	res.failed_layer = -1;
	const int halo = h.is_cfa ? 4 : 2, in_w = SGC_TILE_W + 2 * halo, in_h = SGC_TILE_H + 2 * halo;
	for (int c = 0; c < h.C; c++) {
		uint16_t *plane = frame.data() + (size_t)c * npix;
		/* k_cosme_hist + k_cosme_stat */
		std::vector<uint32_t> hist(65536, 0);
		for (size_t i = 0; i < npix; i++)
			hist[plane[i]]++;
		uint64_t ngood = 0, run = 0, sumabs = 0;
		for (int b = 1; b < 65536; b++)
			ngood += hist[b];
		uint32_t med = 0;
		for (int b = 1; b < 65535; b++) {
			run += hist[b];
			if (2 * run > ngood) {
				med = (uint32_t)b;
				break;
			}
		}
		for (int b = 1; b < 65536; b++)
			sumabs += (uint64_t)hist[b] * (uint64_t)(b > (int)med ? b - (int)med : (int)med - b);
		sgc_rule r;
		sgc_rule_make(&r, (int64_t)ngood, med, sumabs, h.sig0, h.sig1, h.amount, h.is_cfa);
		if (r.ngood <= 0) {
			res.status = 1;
			res.failed_layer = c;
			break;
		}
		res.bkg[c] = r.bkg;
		res.avg_dev[c] = r.avg_dev;
		const size_t words = (npix + 31) / 32;
		std::vector<uint16_t> state(npix, 0xDEAD);
		std::vector<uint32_t> hot(words, 0), cold(words, 0), act[2];
		act[0].assign(words, 0);
		act[1].assign(words, 0);
		std::vector<uint32_t> list[2];
		/* k_cosme_main, tile by tile, each tile in an array of exactly its size */
		for (int y0 = 0; y0 < H; y0 += SGC_TILE_H)
			for (int x0 = 0; x0 < W; x0 += SGC_TILE_W) {
				std::vector<uint16_t> tile((size_t)in_w * in_h);
				for (int idx = 0; idx < in_w * in_h; idx++)
					tile[idx] = sgc_tile_load(idx, plane, W, H, x0, y0, halo);
				SgcTileGet g;
				g.s = tile.data();
				g.x0 = x0;
				g.y0 = y0;
				g.halo = halo;
				g.in_w = in_w;
				std::vector<uint16_t> q1, q2;
				for (int tid = 0; tid < SGC_THREADS; tid++) {
					const int ox = tid % SGC_TILE_W, oy0 = (tid / SGC_TILE_W) * SGC_ROWS, x = x0 + ox;
					if (x >= W)
						continue;
					for (int u = 0; u < SGC_ROWS; u++) {
						const int y = y0 + oy0 + u;
						if (y >= H)
							break;
						const uint32_t pixel = g.at(x, y);
						const int own = sgc_own(r, pixel);
						const uint32_t e = (uint32_t)((oy0 + u) * SGC_TILE_W + ox);
						if (own == SGC_HOT) {
							if ((int32_t)sgc_average(g, W, H, x, y, r.step) <= r.a_max)
								q1.push_back((uint16_t)e);
						} else if (own == SGC_COLD)
							q2.push_back((uint16_t)(e | 0x8000u));
					}
				}
				for (uint16_t e : q1) {
					const int x = x0 + e % SGC_TILE_W, y = y0 + e / SGC_TILE_W;
					if (sgc_hot_maybe(g, W, H, x, y, r, g.at(x, y)))
						q2.push_back(e);
				}
				for (uint16_t e : q2) {
					const uint32_t loc = e & 0x7FFFu;
					const int x = x0 + (int)(loc % SGC_TILE_W), y = y0 + (int)(loc / SGC_TILE_W);
					const uint32_t pixel = g.at(x, y);
					uint16_t val = 0;
					res.medians++;
					const int kind = sgc_decide(g, W, H, x, y, r, pixel, (e & 0x8000u) ? SGC_COLD : SGC_HOT, &val);
					if (kind == SGC_NONE)
						continue;
					const uint32_t gid = (uint32_t)y * W + x;
					state[gid] = val;
					(kind == SGC_HOT ? hot : cold)[gid >> 5] |= 1u << (gid & 31);
					if (val == pixel)
						continue;
					for (int k = 0; k < 12; k++) {
						int xx, yy;
						if (sgc_later(k, x, y, W, H, r.step, &xx, &yy) && sgc_own(r, g.at(xx, yy)) != SGC_NONE) {
							const uint32_t q = (uint32_t)yy * W + xx;
							if (!(act[0][q >> 5] >> (q & 31) & 1u)) {
								act[0][q >> 5] |= 1u << (q & 31);
								list[0].push_back(q);
							}
						}
					}
				}
			}
		/* k_cosme_round until no pixel is listed; the list is walked backwards, so a pixel reads
		 * records already rewritten in its own round: the fixed point does not depend on the order */
		for (int rd = 0; !list[rd & 1].empty(); rd++) {
			res.rounds++;
			const int s = rd & 1, n = (rd + 1) & 1;
			list[n].clear();
			for (size_t i = list[s].size(); i-- > 0;) {
				const uint32_t gid = list[s][i];
				act[s][gid >> 5] &= ~(1u << (gid & 31));
				const uint32_t pixel = plane[gid];
				const int own = sgc_own(r, pixel), x = (int)(gid % W), y = (int)(gid / W);
				const uint32_t w = gid >> 5, bit = 1u << (gid & 31);
				const int oldkind = (hot[w] & bit) ? SGC_HOT : ((cold[w] & bit) ? SGC_COLD : SGC_NONE);
				const uint32_t oldval = oldkind ? state[gid] : pixel;
				SgcStateGet g;
				g.plane = plane;
				g.state = state.data();
				g.hot = hot.data();
				g.cold = cold.data();
				g.base = 0;
				g.p = gid;
				g.W = W;
				uint16_t val = 0;
				int kind = SGC_NONE;
				if (own == SGC_COLD || (own == SGC_HOT && sgc_hot_maybe(g, W, H, x, y, r, pixel)))
					kind = sgc_decide(g, W, H, x, y, r, pixel, own, &val);
				if (kind == SGC_NONE)
					val = (uint16_t)pixel;
				if (kind == oldkind && val == oldval)
					continue;
				if (kind != SGC_NONE)
					state[gid] = val;
				if (oldkind != SGC_NONE && oldkind != kind)
					(oldkind == SGC_HOT ? hot : cold)[w] &= ~bit;
				if (kind != SGC_NONE && oldkind != kind)
					(kind == SGC_HOT ? hot : cold)[w] |= bit;
				for (int k = 0; k < 12; k++) {
					int xx, yy;
					if (sgc_later(k, x, y, W, H, r.step, &xx, &yy) && sgc_own(r, plane[(size_t)yy * W + xx]) != SGC_NONE) {
						const uint32_t q = (uint32_t)yy * W + xx;
						if (!(act[n][q >> 5] >> (q & 31) & 1u)) {
							act[n][q >> 5] |= 1u << (q & 31);
							list[n].push_back(q);
						}
					}
				}
			}
		}
		/* k_cosme_commit */
		for (size_t gid = 0; gid < npix; gid++) {
			const uint32_t bit = 1u << (gid & 31);
			if (hot[gid >> 5] & bit) {
				res.ihot++;
				plane[gid] = state[gid];
			} else if (cold[gid >> 5] & bit) {
				res.icold++;
				plane[gid] = state[gid];
			}
		}
	}
	FILE *fo = fopen(argv[2], "wb");
	if (!fo)
		return 5;
	fwrite(&res, sizeof res, 1, fo);
	fwrite(frame.data(), 2, frame.size(), fo);
	fclose(fo);
	return 0;
}
"""

RES = np.dtype([("status", "<i4"), ("failed_layer", "<i4"), ("icold", "<i8"), ("ihot", "<i8"), ("bkg", "<f8", (3,)),
                ("avg_dev", "<f8", (3,)), ("rounds", "<i8"), ("medians", "<i8")])


def _sanitizer(tmp_path):
    probe = tmp_path / "probe.c"
    probe.write_text("int main(void) { return 0; }\n")
    p = subprocess.run(["gcc", *SAN, str(probe), "-o", str(tmp_path / "probe")], capture_output=True, text=True)
    if p.returncode != 0 or subprocess.run([str(tmp_path / "probe")]).returncode != 0:
        pytest.skip("the AddressSanitizer / UBSan runtime is not installed")
    return SAN


@pytest.fixture(scope="module", params=[False, True], ids=["plain", "asan_ubsan"])
def program(request, tmp_path_factory):
    tmp = tmp_path_factory.mktemp("cosme_host")
    extra, opt = (_sanitizer(tmp), "-O0") if request.param else ([], "-O1")
    src = tmp / "cosme_host.cpp"
    src.write_text(PROGRAM)
    exe = tmp / "cosme_host"
    r = subprocess.run(["g++", opt, "-std=c++17", "-ffp-contract=off", "-fno-fast-math", *extra, "-I", INC, str(src),
                        "-o", str(exe), "-lm"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    return exe, tmp


def _run(program, frame, sig, amount, is_cfa):
    exe, tmp = program
    C, H, W = frame.shape
    with open(tmp / "in.bin", "wb") as f:
        f.write(struct.pack("<iiiiddd", W, H, C, int(is_cfa), float(sig[0]), float(sig[1]), float(amount)))
        f.write(np.ascontiguousarray(frame, dtype=np.uint16).tobytes())
    r = subprocess.run([str(exe), str(tmp / "in.bin"), str(tmp / "out.bin")], capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stderr[-4000:])
    raw = (tmp / "out.bin").read_bytes()
    res = np.frombuffer(raw[:RES.itemsize], dtype=RES)[0]
    out = np.frombuffer(raw[RES.itemsize:], dtype=np.uint16).reshape(C, H, W)
    return out, res


# small shapes, one tile +- 1 both ways and two tiles + 1, chains across tile corners, the dense
# case, truncation, a failing layer: whole frames through the header
HOST_CASES = ["s_1x7", "s_7x1", "s_3x3", "s_5x7_cfa", "s_2x9_cfa", "tile_m1", "tile_p1", "tiles2_p1_cfa", "chain_comb",
              "chain_d", "chain_comb_cfa", "dense", "dense_cfa", "amount_03", "amount_0", "layers3", "fail_layer1",
              "all_65535", "cold_off", "hot_off", "both_off"]


@pytest.mark.parametrize("name", HOST_CASES)
def test_header_program_equals_literal(program, name):
    case = cc.CASES[name]
    for f, frame in enumerate(cc.frames_of(name)):
        want, wres = cc.literal_of(name)[f]
        out, res = _run(program, frame, case["sig"], case["amount"], case["is_cfa"])
        assert np.array_equal(out, want), (name, f, int((out != want).sum()))
        assert (int(res["status"]), int(res["failed_layer"]), int(res["icold"]), int(res["ihot"])) == \
            (wres["status"], wres["failed_layer"], wres["icold"], wres["ihot"]), (name, f, res, wres)
        assert res["bkg"].tolist() == wres["bkg"] and res["avg_dev"].tolist() == wres["avg_dev"]
