"""The host-only plan of a DFT registration call (siril-0.9_amd/csrc/sg_reg_plan.hpp), built for the
host and checked without a GPU: argument errors, the frame and pair lists, the route by side, the
batch counts, strip widths, thread counts and LDS sizes against known answers read from the limits
the code states (8 elements per thread, 1024 threads, 160 KiB of LDS, 2 GB of pair planes), an
invariant sweep over the sides and knob values the GPU tests use, and the host tables (twiddles,
Bluestein's chirp and its spectrum).  A wrong size gives either the right shifts by a slower
route or a launch that fails only at a side no GPU test uses."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INC = os.path.join(ROOT, "siril-0.9_amd", "csrc")
ROCM_INC = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "include")

PROGRAM = r'''
#include <stdio.h>
#include <stdlib.h>
#include <stdint.h>
#include <string.h>
#include <math.h>
#include <vector>
#include "sg_reg_plan.hpp"

static int bad = 0, checks = 0;
#define CHECK(cond) do { checks++; if (!(cond)) { if (bad < 40) printf("FAIL %s:%d: %s\n", __func__, __LINE__, #cond); bad++; } } while (0)

static const size_t LDS_MAX = 160 * 1024;	/* the limit sg_reg_plan tests gen_fuse against */

/* one call to plan: frames, side, reference, mask, the knobs at their defaults */
struct Case {
	int n, S, ref;
	std::vector<int> inc;
	SgKnobs k;
	SgRegPlan pl;
	Case(int S_, int n_ = 7, int ref_ = 0) : n(n_), S(S_), ref(ref_) {}
	int plan() { return sg_reg_plan(n, S, ref, inc.empty() ? nullptr : inc.data(), (int64_t)S * S, S, k, pl); }
};

static bool radices(const SgRegPlan &pl, std::vector<int> want) {
	if (pl.gen.npass != (int)want.size() || pl.gen.n != pl.S)
		return false;
	for (size_t i = 0; i < want.size(); i++)
		if (pl.gen.radix[i] != want[i])
			return false;
	return true;
}

static void test_errors(void) {
	Case a(64, 0);
	CHECK(a.plan() == SG_ERR_GENERIC && !strcmp(a.pl.err, "no frame to register0"));
	Case b(3);
	CHECK(b.plan() == SG_ERR_SIZE && !strcmp(b.pl.err, "DFT registration takes selection sides 4 to 4096 (got 3)"));
	Case c(4097);
	CHECK(c.plan() == SG_ERR_SIZE && !strcmp(c.pl.err, "DFT registration takes selection sides 4 to 4096 (got 4097)"));
	Case d(64, 5, 5);
	CHECK(d.plan() == SG_ERR_GENERIC && !strcmp(d.pl.err, "reference image out of range 5"));
	Case e(64, 5, -1);
	CHECK(e.plan() == SG_OK && e.pl.ref_image == 0 && e.pl.err[0] == 0);
	CHECK(e.pl.hfa[e.pl.NP] == 0 && e.pl.qframes[0] == 0 && e.pl.todo == std::vector<int>({1, 2, 3, 4}));
	Case f(64, 1);
	CHECK(f.plan() == SG_OK && f.pl.npairs_total == 0 && f.pl.NP == 1 && f.pl.todo.empty());
	CHECK(f.pl.hfa == std::vector<int>({0, 0}) && f.pl.hfb == std::vector<int>({0, -1}));
	CHECK(f.pl.B == 64 && f.pl.Bc == 64);	/* no pair to clamp to: the 64-pair cap (the batch loop does not run) */
	CHECK(f.pl.qframes == std::vector<int>({0}));
}

static void test_frames(void) {
	/* seven frames, the reference at 2, frame 4 excluded: five to register, the third pair single */
	Case c(2048, 7, 2);
	c.inc = {1, 1, 1, 1, 0, 1, 1};
	CHECK(c.plan() == SG_OK && c.pl.npairs_total == 3 && c.pl.NP == 3);
	CHECK(c.pl.todo == std::vector<int>({0, 1, 3, 5, 6}));
	CHECK(c.pl.qframes == std::vector<int>({2, 0, 1, 3, 5, 6}));
	CHECK(c.pl.hfa == std::vector<int>({0, 3, 6, 2}) && c.pl.hfb == std::vector<int>({1, 5, -1, -1}));
	CHECK(c.pl.pin_res == 64 && c.pl.pin_bytes == 64 + 3 * 80);
	Case d(64, 9, 8);	/* an even count: no single pair */
	CHECK(d.plan() == SG_OK && d.pl.npairs_total == 4 && d.pl.hfb[3] == 7 && d.pl.hfa[4] == 8 && d.pl.hfb[4] == -1);
	CHECK(d.pl.pin_res == 64 && d.pl.pin_bytes == 64 + 4 * 80);	/* 2 x 5 ints = 40 B, rounded to 64 */
}

static void test_route_by_side(void) {
	for (int S : {4, 6, 7}) {
		Case c(S);
		CHECK(c.plan() == SG_OK && c.pl.generic && c.pl.route == SG_REG_GEN_MIXED && !c.pl.fp32);
	}
	for (int S = 8; S <= 4096; S <<= 1) {
		Case c(S);
		CHECK(c.plan() == SG_OK && !c.pl.generic && c.pl.fp32 && c.pl.tol_main == -15 && c.pl.esz == 8);
		CHECK(c.pl.route == (S == 2048 ? SG_REG_HALF32_WAVE : SG_REG_HALF32_BLOCK) && c.pl.wcol == (S == 2048));
		CHECK(c.pl.gen.npass == 0 && c.pl.tab_total == 4 * (size_t)S && c.pl.logS == (int)lround(log2((double)S)));
		c.k.reg_fp = 64;
		CHECK(c.plan() == SG_OK && c.pl.route == SG_REG_HALF64 && !c.pl.fp32 && c.pl.tol_main == -32 && c.pl.esz == 16);
		CHECK(!c.pl.specp_on && c.pl.qfold == 0);
		c.k.reg_fp = 32;
		c.k.reg_wcol = 0;
		CHECK(c.plan() == SG_OK && c.pl.route == SG_REG_HALF32_BLOCK && !c.pl.wcol && !c.pl.specp_on);
	}
	Case p(64);
	p.k.reg_path = 3;
	CHECK(p.plan() == SG_OK && p.pl.generic && p.pl.route == SG_REG_GEN_MIXED && !p.pl.fp32 && radices(p.pl, {8, 8}));
	Case a(105), b(120), c(48), d(1500);
	CHECK(a.plan() == SG_OK && a.pl.route == SG_REG_GEN_MIXED && radices(a.pl, {3, 5, 7}));
	CHECK(b.plan() == SG_OK && radices(b.pl, {8, 3, 5}));
	CHECK(c.plan() == SG_OK && radices(c.pl, {8, 2, 3}));
	CHECK(d.plan() == SG_OK && radices(d.pl, {4, 3, 5, 5, 5}));
	/* Bluestein: m the power of two >= 2 S - 1, m / 8 threads, m + m / 8 padded fp64 elements */
	const int bs[3] = {97, 1009, 4095}, bm[3] = {256, 2048, 8192}, bt[3] = {64, 256, 1024};
	for (int i = 0; i < 3; i++) {
		Case e(bs[i]);
		CHECK(e.plan() == SG_OK && e.pl.route == SG_REG_GEN_BLUESTEIN && e.pl.gen.bluestein == 1 && e.pl.gen.m == bm[i]);
		CHECK(e.pl.gen_thr == bt[i] && !e.pl.gen_fuse && e.pl.gen_lds == (size_t)(bm[i] + bm[i] / 8) * 16);
		CHECK(e.pl.n_tw == 4 * (size_t)bs[i] && e.pl.n_twm == 4 * (size_t)bm[i] && e.pl.n_ch == 2 * (size_t)bs[i] &&
				e.pl.n_bh == 2 * (size_t)bm[i] && e.pl.tab_total == 6 * (size_t)bs[i] + 6 * (size_t)bm[i]);
		CHECK(e.pl.lds_attrs.size() == 1 && e.pl.lds_attrs[0].kernel == SG_RK_GEN_ROWS_BLUE &&
				e.pl.lds_attrs[0].bytes == (int)e.pl.gen_lds);
	}
}

static void test_generic_fuse(void) {
	/* threads: ceil(S / 8), or ceil(S / 7) with a radix-7 pass, in whole waves; a row is S + S / 8 fp64 elements */
	Case a(105), b(1500), c(2940), d(3920);
	CHECK(a.plan() == SG_OK && a.pl.gen_fuse && a.pl.gen_thr == 64 && a.pl.gen_lds == (size_t)(105 + 13) * 16);
	CHECK(b.plan() == SG_OK && b.pl.gen_fuse && b.pl.gen_thr == 192 && b.pl.gen_lds == 26992);
	CHECK(b.pl.lds_attrs.size() == 2 && b.pl.lds_attrs[0].kernel == SG_RK_GEN_COLS_XPOWER && b.pl.lds_attrs[0].bytes == 2 * 26992 &&
			b.pl.lds_attrs[1].kernel == SG_RK_GEN_ROWS && b.pl.lds_attrs[1].bytes == 26992);
	CHECK(c.plan() == SG_OK && radices(c.pl, {4, 3, 5, 7, 7}) && c.pl.gen_fuse && c.pl.gen_thr == 448);
	CHECK(d.plan() == SG_OK && radices(d.pl, {8, 2, 5, 7, 7}) && d.pl.gen_thr == 576 && !d.pl.gen_fuse);	/* 2 x 576 > 1024 */
	for (Case *p : {&a, &b, &c}) {
		p->k.reg_genfuse = 0;
		CHECK(p->plan() == SG_OK && !p->pl.gen_fuse && p->pl.lds_attrs.size() == 1);
	}
	/* generic planes: the pair and its transpose, fp64 */
	CHECK(b.pl.pair_bytes == (size_t)1500 * 1500 * 32 && b.pl.tgrid == 47);
}

static void test_batching(void) {
	/* 2 GB of pair planes, at most 64 pairs: 2048^2 x 8 B = 32 MiB, x 16 B = 64 MiB, 4096^2 x 8 B = 128 MiB */
	Case a(2048, 200), b(2048, 200), c(4096, 200);
	b.k.reg_fp = 64;
	CHECK(a.plan() == SG_OK && a.pl.npairs_total == 100 && a.pl.B == 64 && a.pl.Bc == 64 && a.pl.B64 == 32);
	CHECK(b.plan() == SG_OK && b.pl.B == 32 && b.pl.B64 == 32);
	CHECK(c.plan() == SG_OK && c.pl.B == 16 && c.pl.B64 == 8);
	Case d(2048, 8);	/* 7 frames to register: 4 pairs */
	CHECK(d.plan() == SG_OK && d.pl.npairs_total == 4 && d.pl.B == 4 && d.pl.B64 == 2 && d.pl.hfb[3] == -1);
	Case e(2048, 3);
	CHECK(e.plan() == SG_OK && e.pl.B == 1 && e.pl.Bc == 1 && e.pl.B64 == 1);	/* max(1, 1 / 2) */
	for (int batch : {1, 2, 3}) {
		Case f(2048, 8);
		f.k.reg_batch = batch;
		CHECK(f.plan() == SG_OK && f.pl.B == batch && f.pl.Bc == batch && f.pl.B64 == (batch / 2 > 1 ? batch / 2 : 1));
	}
	Case g(2048, 8);
	g.k.reg_batch = 100;	/* the knob is clamped to the pairs too */
	CHECK(g.plan() == SG_OK && g.pl.B == 4);
	Case h(60, 8);
	h.k.reg_batch = 1;
	CHECK(h.plan() == SG_OK && h.pl.B == 1 && h.pl.B64 == 1 && h.pl.generic);
}

static void test_strips_and_threads(void) {
	for (int S = 8; S <= 4096; S <<= 1) {
		Case c(S);
		CHECK(c.plan() == SG_OK && c.pl.CW == (S <= 1024 ? 8 : S == 2048 ? 4 : 2) && c.pl.CWh <= S / 2);
		CHECK(c.pl.CWh == (c.pl.CW < S / 2 ? c.pl.CW : S / 2) && (S / 2) % c.pl.CWh == 0);
		/* 8 fp64 elements per thread, at least a wave */
		CHECK(c.pl.row_thr == (S / 8 > 64 ? S / 8 : 64) && c.pl.colh_thr == (c.pl.CWh * S / 8 > 64 ? c.pl.CWh * S / 8 : 64));
		CHECK(c.pl.row_lds == (size_t)(S + S / 8) * 16 && c.pl.row_lds32 == (size_t)(S + S / 8) * 8);
		CHECK(c.pl.colh_lds == (size_t)c.pl.CWh * (S + S / 8 + 1) * 16);
		CHECK(c.pl.colh_lds32 == (size_t)c.pl.CW32 * (S + S / 8 + 4) * 8 && (S / 2) % c.pl.CW32 == 0);
		CHECK(c.pl.wcol_lds == (size_t)4 * 2120 * 8 && c.pl.rpb == 4);
	}
	const int ss[3] = {256, 2048, 4096}, ept[3] = {8, 8, 16}, thr[3] = {128, 1024, 1024};
	for (int i = 0; i < 3; i++) {
		Case c(ss[i]);
		CHECK(c.plan() == SG_OK && c.pl.CW32 == 4 && c.pl.ept32 == ept[i] && c.pl.colh_thr32 == thr[i]);
	}
	Case w(2048);
	w.k.reg_cw32 = 8;
	CHECK(w.plan() == SG_OK && w.pl.CW32 == 8 && w.pl.ept32 == 16 && w.pl.colh_thr32 == 1024);
	Case x(4096);
	x.k.reg_cw32 = 8;	/* 8 x 4096 elements are past the 16 K of a strip */
	CHECK(x.plan() == SG_OK && x.pl.CW32 == 4);
	Case y(8);
	CHECK(y.plan() == SG_OK && y.pl.CW32 == 4 && y.pl.colh_thr32 == 64);
	Case r(2048);
	CHECK(r.plan() == SG_OK && r.pl.rpw == 8 && r.pl.rpb == 4);
	r.k.reg_rpw = 3;
	r.k.reg_rpb = 3;
	CHECK(r.plan() == SG_OK && r.pl.rpw == 1 && r.pl.rpb == 1);
}

static void test_switches(void) {
	Case a(2048);
	CHECK(a.plan() == SG_OK && a.pl.cols32 == SG_COLS32_WAVE8_PERM && a.pl.specp_on && a.pl.qroute == SG_REG_Q_FOLDED && a.pl.qfold == 12);
	CHECK(a.pl.spec_bytes == (size_t)2048 * 2048 * (16 + 8 + 4));
	a.k.reg_wcol = 0;
	CHECK(a.plan() == SG_OK && a.pl.cols32 == SG_COLS32_BLOCK8_OCC && !a.pl.specp_on);
	CHECK(a.pl.spec_bytes == (size_t)2048 * 2048 * 24 && a.pl.qroute == SG_REG_Q_UPFRONT && a.pl.qfold == 0);
	a.k.reg_cw32 = 8;
	CHECK(a.plan() == SG_OK && a.pl.cols32 == SG_COLS32_BLOCK16);
	Case b(256);
	CHECK(b.plan() == SG_OK && b.pl.cols32 == SG_COLS32_BLOCK8_OCC && b.pl.qroute == SG_REG_Q_UPFRONT && b.pl.qfold == 0);
	Case c(4096);
	CHECK(c.plan() == SG_OK && c.pl.cols32 == SG_COLS32_BLOCK16);
	/* the quality route */
	Case f(2048);
	f.k.reg_fp = 64;
	CHECK(f.plan() == SG_OK && f.pl.qroute == SG_REG_Q_UPFRONT && f.pl.qfold == 0);
	f.k.reg_qfold = 0;
	CHECK(f.plan() == SG_OK && f.pl.qroute == SG_REG_Q_UPFRONT);
	f.k.reg_fp = 32;
	CHECK(f.plan() == SG_OK && f.pl.qroute == SG_REG_Q_UPFRONT && f.pl.qfold == 0);
	Case g(2048, 1);	/* no pair: nothing to fold into */
	CHECK(g.plan() == SG_OK && g.pl.qroute == SG_REG_Q_UPFRONT && g.pl.qfold == 0);
	Case i(60);
	CHECK(i.plan() == SG_OK && i.pl.qroute == SG_REG_Q_UPFRONT);
}

/* the knobs of the removed A/B variants are no longer read: each set to its old losing value, SgKnobs::read() gives
 * the default plan.  same_plan lists the decisions by hand: a field added to SgRegPlan belongs here too */
#define EQ(f) (a.f == b.f)
static bool same_plan(const SgRegPlan &a, const SgRegPlan &b) {
	auto attr = [](const SgRegLdsAttr &x, const SgRegLdsAttr &y) { return x.kernel == y.kernel && x.bytes == y.bytes; };
	return std::equal(a.lds_attrs.begin(), a.lds_attrs.end(), b.lds_attrs.begin(), b.lds_attrs.end(), attr) &&
		EQ(npairs_total) && EQ(NP) && EQ(route) && EQ(generic) && EQ(fp32) && EQ(wcol) && !memcmp(&a.gen, &b.gen, sizeof a.gen) &&
		EQ(gen_thr) && EQ(gen_lds) && EQ(gen_fuse) && EQ(plane) && EQ(esz) && EQ(pair_bytes) && EQ(B) && EQ(Bc) && EQ(B64) &&
		EQ(row_thr) && EQ(row_lds) && EQ(row_lds32) && EQ(CW) && EQ(CWh) && EQ(colh_thr) && EQ(colh_lds) && EQ(CW32) &&
		EQ(ept32) && EQ(colh_thr32) && EQ(colh_lds32) && EQ(wcol_lds) && EQ(rpw) && EQ(rpb) && EQ(logS) && EQ(tol_main) &&
		EQ(tgrid) && EQ(cols32) && EQ(qroute) && EQ(qfold) && EQ(specp_on) && EQ(n_tw) && EQ(n_twm) && EQ(n_ch) && EQ(n_bh) &&
		EQ(tab_total) && EQ(spec_bytes) && EQ(work_bytes) && EQ(o_out) && EQ(o_fab) && EQ(o_en) && EQ(o_cand) && EQ(o_res2) &&
		EQ(ws) && EQ(pin_res) && EQ(pin_bytes);
}
static void test_removed_knobs(void) {
	const char *knobs[9][2] = {{"SG_REG_SPECP", "0"}, {"SG_REG_WCOLW", "4"}, {"SG_REG_XCD", "0"}, {"SG_REG_PB", "4"},
		{"SG_REG_QAFTER", "1"}, {"SG_QGRAD_STREAM", "0"}, {"SG_QGRAD_THREADS", "256"}, {"SG_REG_REFCONC", "0"},
		{"SG_REG_COLOCC", "0"}};
	for (auto &kv : knobs)
		setenv(kv[0], kv[1], 1);
	for (int S : {2048, 1024, 256}) {
		Case def(S), set(S);	/* def: the knobs as constructed */
		set.k.read();
		CHECK(def.plan() == SG_OK && set.plan() == SG_OK && same_plan(def.pl, set.pl) && set.pl.lds_attrs.size() == 16);
		CHECK(set.pl.cols32 == (S == 2048 ? SG_COLS32_WAVE8_PERM : SG_COLS32_BLOCK8_OCC) && set.pl.qfold == (S == 2048 ? 12 : 0));
	}
}

/* ---- the invariant sweep ---- */
static bool thr_ok(int t) { return t >= 64 && t <= 1024 && t % 64 == 0; }

static void check_invariants(Case &c) {
	CHECK(c.plan() == SG_OK);
	const SgRegPlan &pl = c.pl;
	const int S = pl.S, NP = pl.NP, Bm = pl.Bc > pl.B64 ? pl.Bc : pl.B64;
	if (pl.generic) {
		CHECK(thr_ok(pl.gen_thr) && pl.gen_lds <= LDS_MAX);
		CHECK(!pl.gen_fuse || (thr_ok(2 * pl.gen_thr) && 2 * pl.gen_lds <= LDS_MAX));
		CHECK((pl.route == SG_REG_GEN_BLUESTEIN) == (pl.gen.bluestein != 0));
		if (!pl.gen.bluestein) {	/* the radices multiply to S */
			long prod = 1;
			for (int q = 0; q < pl.gen.npass; q++)
				prod *= pl.gen.radix[q];
			CHECK(prod == S && pl.gen_lds == pl.row_lds);
		} else {
			CHECK(pl.gen.m >= 2 * S - 1 && pl.gen.m < 2 * (2 * S - 1) && (pl.gen.m & (pl.gen.m - 1)) == 0);
			CHECK(pl.gen.m / 8 <= pl.gen_thr);
		}
	} else {
		CHECK(thr_ok(pl.row_thr) && thr_ok(pl.colh_thr) && (!pl.fp32 || thr_ok(pl.colh_thr32)));
		CHECK(pl.row_lds <= LDS_MAX && pl.colh_lds <= LDS_MAX && pl.row_lds32 <= LDS_MAX && pl.colh_lds32 <= LDS_MAX);
		CHECK(2 * pl.wcol_lds <= LDS_MAX);
		CHECK(S % pl.rpb == 0 && (S / 4) % pl.rpw == 0 && (S / 2) % pl.CWh == 0 && (S / 2) % pl.CW32 == 0);
		CHECK(pl.CWh * S <= 8 * pl.colh_thr && (!pl.fp32 || pl.CW32 * S <= pl.ept32 * pl.colh_thr32));
		CHECK(pl.wcol == (S == 2048 && c.k.reg_wcol));
	}
	for (const SgRegLdsAttr &a : pl.lds_attrs)
		CHECK(a.kernel >= 0 && a.kernel < SG_RK_COUNT && a.bytes > 0 && (size_t)a.bytes <= LDS_MAX);
	/* the workspace: each region holds what is carved from it, in order, 256-aligned */
	CHECK(pl.o_out % 256 == 0 && pl.o_fab % 256 == 0 && pl.o_en % 256 == 0 && pl.o_cand % 256 == 0 && pl.o_res2 % 256 == 0);
	CHECK(pl.o_out >= (size_t)Bm * S * SG_REG_SIZEOF_BEST);
	CHECK(pl.o_fab >= pl.o_out + (size_t)(NP + 1) * SG_REG_SIZEOF_OUT);
	CHECK(pl.o_en >= pl.o_fab + (size_t)4 * (NP + 1) * sizeof(int));
	CHECK(pl.o_cand >= pl.o_en + (size_t)2 * pl.nframes * sizeof(unsigned long long));
	CHECK(pl.o_res2 >= pl.o_cand + (size_t)2 * Bm * SG_REG_SIZEOF_CAND);
	CHECK(pl.ws == pl.o_res2 + (size_t)(NP + 1) * SG_REG_SIZEOF_OUT);
	CHECK(pl.work_bytes >= (size_t)pl.Bc * pl.pair_bytes && pl.work_bytes >= (size_t)pl.B64 * pl.plane * 16);
	CHECK(pl.pair_bytes == pl.plane * pl.esz * (pl.generic ? 2 : 1) && pl.B >= 1 && pl.Bc >= 1 && pl.B64 >= 1);
	CHECK(pl.spec_bytes >= pl.plane * 16 + (pl.fp32 ? pl.plane * 8 : 0) + (pl.specp_on ? pl.plane * 4 : 0));
	CHECK(pl.pin_res % 64 == 0 && pl.pin_res >= (size_t)2 * (NP + 1) * sizeof(int) &&
			pl.pin_bytes == pl.pin_res + (size_t)NP * SG_REG_SIZEOF_OUT);
	CHECK((pl.qroute == SG_REG_Q_FOLDED) == (pl.qfold != 0));
}

struct KnobSet { int path, genfuse, wcol, fp, qfold, batch, cw32; };

static void test_sweep(void) {
	std::vector<int> sides;
	for (int S = 4; S <= 4096; S <<= 1)
		sides.push_back(S);
	const int other[40] = {5, 6, 7, 9, 10, 11, 12, 15, 24, 35, 48, 60, 63, 65, 97, 100, 105, 120, 127, 129, 255, 257, 360,
		500, 511, 513, 1000, 1009, 1023, 1025, 1234, 1500, 2047, 2049, 2940, 3000, 3072, 3920, 4094, 4095};
	sides.insert(sides.end(), other, other + 40);
	/* the defaults, then each knob value a GPU test sets */
	const KnobSet sets[] = {
		{2, 1, 1, 32, 12, 0, 4}, {3, 1, 1, 32, 12, 0, 4}, {2, 0, 1, 32, 12, 0, 4}, {2, 1, 0, 32, 12, 0, 4},
		{2, 1, 1, 64, 12, 0, 4}, {3, 1, 1, 64, 12, 0, 4}, {2, 1, 1, 32, 0, 0, 4}, {2, 1, 1, 32, 3, 0, 4},
		{2, 1, 1, 32, 6, 0, 4}, {2, 1, 1, 32, 12, 1, 4}, {2, 1, 1, 32, 12, 2, 4}, {2, 1, 0, 32, 12, 0, 8}};
	int planned = 0;
	for (int S : sides)
		for (const KnobSet &ks : sets)
			for (int shape = 0; shape < 3; shape++) {	/* the GPU tests' seven frames, one frame, many */
				Case c(S, shape == 0 ? 7 : shape == 1 ? 1 : 150, shape == 0 ? 2 : 0);
				if (shape == 0)
					c.inc = {1, 1, 1, 1, 0, 1, 1};
				c.k.reg_path = ks.path, c.k.reg_genfuse = ks.genfuse, c.k.reg_wcol = ks.wcol, c.k.reg_fp = ks.fp;
				c.k.reg_qfold = ks.qfold, c.k.reg_batch = ks.batch, c.k.reg_cw32 = ks.cw32;
				check_invariants(c);
				planned++;
			}
	CHECK(planned == (11 + 40) * 12 * 3);
}

/* ---- the host tables ---- */
static void test_twiddles(void) {
	for (int n : {8, 64, 60}) {
		std::vector<double> tw;
		make_twiddles(n, tw);
		CHECK(tw.size() == 4 * (size_t)n && tw[0] == 1.0 && tw[1] == 0.0);
		for (int k = 0; k < n; k++) {
			CHECK(tw[2 * (n + k)] == tw[2 * k] && tw[2 * (n + k) + 1] == -tw[2 * k + 1]);
			/* a rounded cos / sin of a rounded angle below 2 pi: see CHIRP_TOL */
			CHECK(fabsl((long double)tw[2 * k] - cosl(-2.0L * M_PIl * k / n)) < 4e-15L);
			CHECK(fabsl((long double)tw[2 * k + 1] - sinl(-2.0L * M_PIl * k / n)) < 4e-15L);
		}
		if ((n & (n - 1)) == 0)
			for (int k = 0; k < n / 2; k++)
				CHECK(tw[2 * (k + n / 2)] == -tw[2 * k] && tw[2 * (k + n / 2) + 1] == -tw[2 * k + 1]);
		std::vector<float> t32;
		make_twiddles32(n, t32);
		CHECK(t32.size() == tw.size());
		for (size_t i = 0; i < tw.size(); i++)
			CHECK(t32[i] == (float)tw[i]);
	}
}

static void test_bluestein(void) {
	const int S = 11, m = 32;
	Case c(S);
	CHECK(c.plan() == SG_OK && c.pl.gen.bluestein && c.pl.gen.m == m);
	std::vector<double> ch, bh;
	make_bluestein(S, m, ch, bh);
	CHECK(ch.size() == 2 * (size_t)S && bh.size() == 2 * (size_t)m);
	/* the angle a = -M_PI q / S, |a| < 2 pi, carries M_PI's own error (1.2e-16 / pi relative) and
	 * two roundings: |da| <= 2 pi (3.9e-17 + 2 x 1.11e-16) = 1.7e-15; cos / sin move by at most
	 * |da| and are rounded once more (1.1e-16): below 4e-15 */
	const long double CHIRP_TOL = 4e-15L;
	for (int j = 0; j < S; j++) {
		const long double a = -M_PIl * (long double)(((long long)j * j) % (2 * S)) / (long double)S;
		CHECK(fabsl((long double)ch[2 * j] - cosl(a)) < CHIRP_TOL && fabsl((long double)ch[2 * j + 1] - sinl(a)) < CHIRP_TOL);
	}
	/* b as the plan builds it from its own chirp: b_j = b_{m - j} = conj c_j */
	std::vector<long double> br(m, 0.0L), bi(m, 0.0L);
	for (int j = 0; j < S; j++) {
		br[j] = ch[2 * j];
		bi[j] = -ch[2 * j + 1];
		if (j) {
			br[m - j] = br[j];
			bi[m - j] = bi[j];
		}
	}
	/* host_fft_pow2 in double over log2(m) stages: a stage's output is the sum of two values of
	 * magnitude <= 2^t (unit-magnitude inputs), one of them times a twiddle whose components are
	 * off by at most 8 u (the angle's 6.7 u at |a| <= pi, the rounded cos / sin; u = 2^-53); with
	 * the product's and the sum's own roundings a stage adds at most 20 u 2^t to an entry and
	 * doubles what it inherits: e_t <= 2 e_(t-1) + 20 u 2^t, so e <= 20 u m log2(m) at the end */
	const long double BHAT_TOL = 20.0L * ldexpl(1.0L, -53) * m * 5;
	for (int k = 0; k < m; k++) {
		long double sr = 0.0L, si = 0.0L;
		for (int j = 0; j < m; j++) {
			const long double a = -2.0L * M_PIl * (long double)((k * j) % m) / (long double)m;
			sr += br[j] * cosl(a) - bi[j] * sinl(a);
			si += br[j] * sinl(a) + bi[j] * cosl(a);
		}
		CHECK(fabsl((long double)bh[2 * k] - sr) < BHAT_TOL && fabsl((long double)bh[2 * k + 1] - si) < BHAT_TOL);
	}
	std::vector<double> twm;
	make_twiddles(m, twm);
	CHECK(twm.size() == c.pl.n_twm && ch.size() == c.pl.n_ch && bh.size() == c.pl.n_bh);
}

int main(void) {
	test_errors();
	test_frames();
	test_route_by_side();
	test_generic_fuse();
	test_batching();
	test_strips_and_threads();
	test_switches();
	test_sweep();
	test_twiddles();
	test_bluestein();
	test_removed_knobs();	/* last: it leaves the variables set */
	printf("checks=%d bad=%d\n", checks, bad);
	return bad != 0;
}
'''


def _build(tmp_path, extra, opt="-O1"):
    src = tmp_path / "reg_plan_check.cpp"
    src.write_text(PROGRAM)
    exe = tmp_path / "reg_plan_check"
    r = subprocess.run(["g++", opt, "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-D__HIP_PLATFORM_AMD__", *extra,
                        "-I", INC, "-I", ROCM_INC, str(src), "-o", str(exe), "-lm"],
                       capture_output=True, text=True)
    return exe, r


def _run(exe):
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    assert " bad=0" in r.stdout and "checks=" in r.stdout, r.stdout[-2000:]


def test_reg_plan_known_answers_and_invariants(tmp_path):
    exe, r = _build(tmp_path, [])
    assert r.returncode == 0, r.stderr[-4000:]
    _run(exe)


def test_reg_plan_sanitized(tmp_path):
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
