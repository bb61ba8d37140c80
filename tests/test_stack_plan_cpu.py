"""The host-only plan of a stacking call (siril-0.9_amd/csrc/sg_stack_plan.hpp), built for the host
and checked without a GPU: the chain tables against the oracle's block partition, the additive fold
and the border-row table against or_round_to_WORD, and the kernel choice against known answers read
from the limits the kernels state (N = 16 / 1024 / 2048 / 65535, the 2^30 / 2^31 plane offsets,
|shiftx| <= 16383, the 384 MiB compact cap, KM 8 / 16).  A wrong choice sends a stack down a slower
but still exact path, which no parity test on the GPU sees."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INC = os.path.join(ROOT, "siril-0.9_amd", "csrc")
ORC = os.path.join(ROOT, "oracle")
ORC_CFLAGS = ["-O2", "-fopenmp", "-fPIC", "-ffp-contract=off", "-fno-fast-math"]    # oracle/Makefile
ROCM_INC = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "include")

PROGRAM = r'''
#include <stdio.h>
#include <stdlib.h>
#include <stdint.h>
#include <string.h>
#include <math.h>
#include <vector>
#include "sg_stack_plan.hpp"
extern "C" {
#include "oracle.h"
}

static int bad = 0, checks = 0;
#define CHECK(cond) do { checks++; if (!(cond)) { if (bad < 40) printf("FAIL %s:%d: %s\n", __func__, __LINE__, #cond); bad++; } } while (0)

static uint64_t s = 88172645463325252ull;
static uint64_t rnd(void) { s ^= s << 13; s ^= s >> 7; s ^= s << 17; return s; }
static double uni(double a, double b) { return a + (b - a) * ((double)(rnd() >> 11) / 9007199254740992.0); }
static int irange(int a, int b) { return a + (int)(rnd() % (uint64_t)(b - a + 1)); }	/* [a, b] */

/* one stack to plan: the descriptor, its arrays, the knobs at their defaults */
struct Case {
	sg_stack_desc d;
	SgKnobs k;
	SgStackPlan pl;
	std::vector<int> sx, sy;
	std::vector<double> off, mul, sc;
	Case(int method, int rejection, int N, int W = 256, int H = 8, int C = 1) {
		memset(&d, 0, sizeof d);
		d.method = method;
		d.rejection = rejection;
		d.nb_frames = N;
		d.width = W;
		d.height = H;
		d.nb_layers = C;
		d.sig[0] = 4.0;
		d.sig[1] = 3.0;
		d.max_thread = 4;
		d.max_number_of_rows = H;
	}
	void shifts() {
		sx.assign(d.nb_frames, 0);
		sy.assign(d.nb_frames, 0);
		d.shiftx = sx.data();
		d.shifty = sy.data();
	}
	void norm(int mode) {
		d.normalize = mode;
		off.assign(d.nb_frames, 0.5);
		mul.assign(d.nb_frames, 1.0);
		sc.assign(d.nb_frames, 1.0);
		d.offset = off.data();
		d.mul = mul.data();
		d.scale = sc.data();
	}
	int plan() { return sg_stack_plan(&d, 0, d.height, k, pl); }
	int plan(int rb, int re) { return sg_stack_plan(&d, rb, re, k, pl); }
};

/* ---- chain tables against the reference's partition ---- */
static void test_chain_tables(void) {
	const int Hs[] = {1, 2, 7, 24, 100}, Cs[] = {1, 3}, Ts[] = {1, 2, 3, 4, 8, 16};
	int failed = 0, ok = 0;
	for (int H : Hs) for (int C : Cs) for (int T : Ts) {
		const int Rs[] = {0, 1, 5, H};
		for (int R : Rs) {
			std::vector<or_block> ob(4096);
			const int nb = or_make_blocks(H, C, R > 0 ? R : H, T, ob.data(), (int)ob.size());
			Case c(SG_STACK_MEAN, SG_SIGMA, 8, 64, H, C);
			c.d.max_thread = T;
			c.d.max_number_of_rows = R;
			const int rc = c.plan();
			Case m(SG_STACK_MEAN, SG_NO_REJEC, 8, 64, H, C);	/* no rejection: a failed partition is ignored */
			m.d.max_thread = T;
			m.d.max_number_of_rows = R;
			CHECK(m.plan() == SG_OK && m.pl.tables.empty() && m.pl.nblocks == 0);
			if (nb < 0) {
				failed++;
				CHECK(rc == SG_ERR_GENERIC);
				CHECK(!strcmp(c.pl.err, "block partition failed (the reference would read uninitialised blocks)0"));
				continue;
			}
			ok++;
			CHECK(rc == SG_OK && c.pl.nblocks == nb);
			if (rc != SG_OK || c.pl.nblocks != nb)
				continue;
			CHECK(c.pl.tables.size() == (size_t)C * H + 4 * (size_t)nb);
			const int *row = c.pl.tables.data(), *bch = row + (size_t)C * H, *bst = bch + nb, *ben = bst + nb, *bfi = ben + nb;
			for (int b = 0; b < nb; b++) {
				CHECK(bch[b] == ob[b].channel && bst[b] == ob[b].start_row && ben[b] == ob[b].end_row);
				for (long r = ob[b].start_row; r <= ob[b].end_row; r++)
					CHECK(row[(size_t)ob[b].channel * H + r] == b);
			}
			for (int t = 0; t < T; t++) {
				long b0, b1;
				or_omp_static_chunk(nb, T, t, &b0, &b1);
				for (long b = b0; b < b1; b++)
					CHECK(bfi[b] == (int)b0);
			}
		}
	}
	CHECK(failed > 0 && ok > 100);
}

/* ---- the additive fold ---- */
static double family_offset(int kind) {	/* the offset families of tests/test_norm_fold.py */
	switch (kind) {
	case 0: return uni(-200, 200);
	case 1: return (double)irange(-200, 199) + 0.5;
	case 2: return (double)irange(-200, 199) + 0.5 + (rnd() & 1 ? 1.0 : -1.0) * ldexp(1.0, -irange(20, 51));
	case 3: return uni(-2000, 2000) * ldexp(1.0, -irange(0, 11));
	default: return nextafter((double)irange(-300, 299) + 0.5, rnd() & 1 ? 1e9 : -1e9);
	}
}

/* offset - 0.5 is a double: the difference, put back, gives the offset again (80-bit arithmetic) */
static bool half_exact(double b) {
	const double c = b - 0.5;
	return (long double)c + 0.5L == (long double)b;
}

static void check_fold_set(Case &c, int expect_fold) {
	const int N = c.d.nb_frames;
	CHECK(c.plan() == SG_OK);
	bool all = true;
	for (int i = 0; i < N; i++)
		all = all && half_exact(c.off[i]);
	CHECK(c.pl.hist_norm_fold == (all ? 1 : 0));
	if (expect_fold >= 0)
		CHECK(c.pl.hist_norm_fold == expect_fold);
	CHECK(c.pl.norm == (c.pl.hist_norm_fold ? 3 : 1));
	const double *pair = c.pl.nm.data() + 3 * N;
	for (int i = 0; i < N; i++) {
		CHECK(pair[2 * i] == c.sc[i]);
		if (!c.pl.hist_norm_fold) {
			CHECK(pair[2 * i + 1] == c.off[i]);
			continue;
		}
		CHECK((long double)pair[2 * i + 1] + 0.5L == (long double)c.off[i]);
		int diff = 0;
		for (int v = 0; v < 65536; v++) {
			const double z = (double)v * pair[2 * i] - pair[2 * i + 1];
			const double t = trunc(z > 0.0 ? z : 0.0);
			const int folded = t > 65535.0 ? 65535 : (int)t;
			diff += folded != (int)or_round_to_WORD((double)v * c.sc[i] - c.off[i]);
		}
		CHECK(diff == 0);
	}
}

static void test_additive_fold(int nsets) {
	int folded = 0;
	for (int t = 0; t < nsets; t++) {
		const int N = irange(2, 9);
		Case c(SG_STACK_MEAN, SG_SIGMA, N);
		c.norm(t & 1 ? SG_ADDITIVE : SG_ADDITIVE_SCALING);
		for (int i = 0; i < N; i++) {
			c.off[i] = family_offset(t % 4 == 3 ? (int)(rnd() % 5) : t % 5);
			c.sc[i] = t % 3 ? uni(0.5, 2.0) : 1.0 + (double)irange(-3, 3) * ldexp(1.0, -irange(1, 29));
		}
		check_fold_set(c, -1);
		folded += c.pl.hist_norm_fold;
	}
	CHECK(folded > nsets / 5 && folded < nsets);
	/* one offset of 1e-30 among half-integers: no fold, the pairs hold the offsets themselves */
	Case c(SG_STACK_MEAN, SG_SIGMA, 36);
	c.norm(SG_ADDITIVE_SCALING);
	for (int i = 0; i < 36; i++)
		c.off[i] = (double)irange(-120, 120) / 2.0;
	check_fold_set(c, 1);
	c.off[5] = 1e-30;
	check_fold_set(c, 0);
}

/* ---- the border-row table ---- */
static void check_ztab(Case &c, int k1, int k2, bool expect_entries) {
	const int N = c.d.nb_frames, H = c.d.height;
	CHECK(c.plan() == SG_OK);
	std::vector<int> z((size_t)8 * (k1 + k2), 0);
	bool any = false;
	for (int t = 0; t < k1 + k2; t++) {
		const int R = t < k1 ? t : H - k2 + (t - k1);
		long long n = 0, sum = 0, sq = 0, lo = 65535, hi = 0;
		for (int f = 0; f < N; f++) {
			if (R - c.sy[f] >= 0 && R - c.sy[f] < H)
				continue;
			const long long w = or_round_to_WORD(0.0 * c.sc[f] - c.off[f]);
			if (w == 0 || w == 65535)
				continue;
			n++, sum += w, sq += w * w, lo = w < lo ? w : lo, hi = w > hi ? w : hi;
		}
		if (!n)
			continue;
		any = true;
		int *e = &z[(size_t)8 * t];
		e[0] = (int)n, e[1] = (int)(uint32_t)sum, e[6] = (int)(sum >> 32), e[2] = (int)(uint32_t)sq, e[3] = (int)(sq >> 32);
		e[4] = (int)lo, e[5] = (int)hi;
	}
	CHECK(any == expect_entries);
	if (!any) {
		CHECK(c.pl.ztab.empty() && c.pl.ztab_k1 == 0 && c.pl.ztab_k2 == 0);
		return;
	}
	CHECK(c.pl.ztab_k1 == k1 && c.pl.ztab_k2 == k2);
	CHECK(c.pl.ztab == z);
}

static void test_ztab(void) {
	const int sy[5] = {0, 3, -3, 1, -2};
	const double off[5] = {-100.3, -7.25, -300.5, -0.2, -65600.0};	/* zeros 100, 7, 301, 0 and 65535 (the last two left out) */
	for (int H : {12, 4}) {
		Case c(SG_STACK_MEAN, SG_SIGMA, 5, 64, H);
		c.shifts();
		c.norm(SG_ADDITIVE_SCALING);
		for (int i = 0; i < 5; i++) {
			c.sy[i] = sy[i];
			c.off[i] = off[i];
			c.sc[i] = 1.0 + 0.01 * i;
		}
		if (H == 12)
			check_ztab(c, 3, 3, true);
		else
			check_ztab(c, 4, 0, true);	/* k1 + k2 >= H: every row is a border row */
		for (int i = 0; i < 5; i++)
			c.off[i] = 0.25 * i;	/* offsets >= 0: every normalised zero is 0 */
		check_ztab(c, H == 12 ? 3 : 4, H == 12 ? 3 : 0, false);
		for (int i = 0; i < 5; i++)
			c.off[i] = off[i];
		c.d.normalize = SG_MULTIPLICATIVE_SCALING;
		CHECK(c.plan() == SG_OK && c.pl.ztab.empty() && c.pl.ztab_k1 == 0 && c.pl.ztab_k2 == 0);
		c.d.normalize = SG_ADDITIVE;
		c.d.shiftx = c.d.shifty = nullptr;
		CHECK(c.plan() == SG_OK && c.pl.ztab.empty() && c.pl.ztab_k1 == 0 && c.pl.ztab_k2 == 0);
	}
}

/* ---- route known answers ---- */
static void test_route_n15_n16(void) {
	const int rej[5] = {SG_SIGMA, SG_WINSORIZED, SG_PERCENTILE, SG_SIGMEDIAN, -1}, rj[5] = {2, 4, 1, 3, 8};
	for (int i = 0; i < 5; i++) {
		const int method = rej[i] < 0 ? SG_STACK_MEDIAN : SG_STACK_MEAN, r = rej[i] < 0 ? SG_NO_REJEC : rej[i];
		Case a(method, r, 15);
		CHECK(a.plan() == SG_OK && a.pl.main == SG_MAIN_SORTED && a.pl.nreg == 1 && a.pl.path == 0);
		CHECK(a.pl.redo == SG_REDO_NONE && a.pl.main_kernel_blocks == 4 * 8 && a.pl.main_grid[0] == 32);
		CHECK(a.pl.main_lds == (size_t)15 * 66 * 2 && a.pl.main_threads == 256);
		Case b(method, r, 16);
		CHECK(b.plan() == SG_OK && b.pl.main == SG_MAIN_HIST && b.pl.rj == rj[i] && b.pl.norm == 0);
		CHECK(b.pl.path == 1 && b.pl.main_grid[0] == 2 * 8 && b.pl.main_kernel_blocks == 4 * 8 && b.pl.main_lds == 0);
		/* launches: main, redo, the replay (SIGMA / WINSORIZED only), two literal phases */
		CHECK(b.pl.launches == (i < 2 ? 5 : 4));
		CHECK(a.pl.launches == (i < 2 ? 4 : 3));
		b.d.kernel_path = SG_PATH_SORTED;
		CHECK(b.plan() == SG_OK && b.pl.main == SG_MAIN_SORTED);
	}
	for (int N : {16, 700, 1024}) {
		Case c(SG_STACK_MEAN, SG_SIGMA, N);
		c.d.kernel_path = SG_PATH_SORTED;
		CHECK(c.plan() == SG_OK && c.pl.main == SG_MAIN_SORTED);
	}
	Case sm(SG_STACK_MEAN, SG_SIGMEDIAN, 64);
	sm.k.hist_sigmedian = 0;
	CHECK(sm.plan() == SG_OK && sm.pl.main == SG_MAIN_SORTED);
	const int ns[] = {2, 64, 65, 128, 129, 256, 257, 512, 513, 1024, 1025}, nr[] = {1, 1, 2, 2, 4, 4, 8, 8, 16, 16, 0};
	for (int i = 0; i < 11; i++) {
		Case c(SG_STACK_MEAN, SG_SIGMA, ns[i]);
		CHECK(c.plan() == SG_OK && c.pl.nreg == nr[i] && pick_nreg(ns[i]) == nr[i]);
	}
}

static void test_route_linfit(void) {
	for (int N : {16, 512, 513, 1024}) {
		const int km = N <= 512 ? 8 : 16;
		Case c(SG_STACK_MEAN, SG_LINEARFIT, N);
		CHECK(c.plan() == SG_OK && c.pl.main == SG_MAIN_LINFIT && c.pl.km == km && c.pl.nw == 8);
		CHECK(c.pl.path == 1 && c.pl.redo == SG_REDO_SORTED && c.pl.replay_nm == 0 && c.pl.linfit_tables);
		CHECK(c.pl.main_grid[0] == 4 * 8 && c.pl.main_threads == 512);
		CHECK(c.pl.main_lds == (size_t)64 * (64 * km + 2) * 2 && c.pl.launches == 4 && !c.pl.compact);
		CHECK(c.pl.sorted_lds == (size_t)N * 66 * 2 + (size_t)64 * ((N + 31) / 32) * 4);
		c.k.linfit_waves = 4;
		CHECK(c.plan() == SG_OK && c.pl.nw == 4 && c.pl.main_threads == 256);
		c.k.linfit_waves = 16;
		CHECK(c.plan() == SG_OK && c.pl.nw == (km == 8 ? 16 : 8));
		c.k.linfit_waves = 12;
		CHECK(c.plan() == SG_OK && c.pl.nw == 8);
	}
	Case a(SG_STACK_MEAN, SG_LINEARFIT, 15);
	CHECK(a.plan() == SG_OK && a.pl.main == SG_MAIN_SORTED && a.pl.linfit_tables);
	CHECK(a.pl.main_lds == (size_t)15 * 66 * 2 + 64 * 4);
	Case b(SG_STACK_MEAN, SG_LINEARFIT, 1025);
	CHECK(b.plan() == SG_OK && b.pl.main == SG_MAIN_LITERAL_ALL && b.pl.main_kernel_blocks == 0 && b.pl.launches == 3);
	Case f(SG_STACK_MEAN, SG_LINEARFIT, 64);
	f.k.linfit_fast = 0;
	CHECK(f.plan() == SG_OK && f.pl.main == SG_MAIN_SORTED);
	f.k.linfit_fast = 1;
	f.d.kernel_path = SG_PATH_SORTED;
	CHECK(f.plan() == SG_OK && f.pl.main == SG_MAIN_SORTED);
}

static void test_route_large_n(void) {
	Case a(SG_STACK_MEAN, SG_SIGMA, 1025);
	a.norm(SG_ADDITIVE_SCALING);
	CHECK(a.plan() == SG_OK && a.pl.main == SG_MAIN_HIST && a.pl.redo == SG_REDO_TO_LITERAL && !a.pl.compact);
	CHECK(a.pl.replay_nm == SG_REPLAY_MAXN && a.pl.list_minn == 0 && a.pl.rp_maxn == 0 && a.pl.launches == 5);
	a.d.kernel_path = SG_PATH_SORTED;
	CHECK(a.plan() == SG_OK && a.pl.main == SG_MAIN_LITERAL_ALL && a.pl.replay_nm == SG_REPLAY_MAXN);
	Case b(SG_STACK_MEAN, SG_SIGMA, 2049);
	CHECK(b.plan() == SG_OK && b.pl.main == SG_MAIN_HIST && b.pl.replay_nm == 0 && b.pl.launches == 4);
	Case c(SG_STACK_MEAN, SG_SIGMA, 2048);
	CHECK(c.plan() == SG_OK && c.pl.replay_nm == SG_REPLAY_MAXN && c.pl.redo == SG_REDO_TO_LITERAL);
	Case d(SG_STACK_MEAN, SG_WINSORIZED, 65535, 64, 4);
	CHECK(d.plan() == SG_OK && d.pl.main == SG_MAIN_HIST && d.pl.rj == 4);
	Case e(SG_STACK_MEAN, SG_WINSORIZED, 65536, 64, 4);
	CHECK(e.plan() == SG_OK && e.pl.main == SG_MAIN_LITERAL_ALL);
	/* k_stack_literal: SG_LIT_THREADS threads while 1 GiB of scratch holds them */
	CHECK(c.pl.lit_threads == SG_LIT_THREADS && c.pl.scratch_bytes == (size_t)SG_LIT_THREADS * 10240);
	CHECK(e.pl.lit_threads == 4096 && e.pl.scratch_bytes == (size_t)4096 * 327680);
}

static void test_route_replay(void) {
	for (int rej : {SG_SIGMA, SG_WINSORIZED, SG_PERCENTILE, SG_SIGMEDIAN}) {
		const bool sw = rej == SG_SIGMA || rej == SG_WINSORIZED;
		for (int N : {16, 512, 513, 1024}) {
			Case c(SG_STACK_MEAN, rej, N);
			CHECK(c.plan() == SG_OK && c.pl.main == SG_MAIN_HIST);
			CHECK(c.pl.redo == (sw ? SG_REDO_REPLAY_THEN_SORTED : SG_REDO_SORTED));
			CHECK(c.pl.list_minn == (sw ? SG_REDO_REPLAY_MAX : 0u) && c.pl.rp_maxn == c.pl.list_minn);
			CHECK(c.pl.replay_nm == (sw ? (N <= 512 ? 512 : SG_REPLAY_MAXN) : 0));
			c.k.redo_replay = 0;
			CHECK(c.plan() == SG_OK && c.pl.redo == SG_REDO_SORTED && c.pl.list_minn == 0 && c.pl.rp_maxn == 0);
			CHECK(c.pl.replay_nm == (sw ? (N <= 512 ? 512 : SG_REPLAY_MAXN) : 0));
		}
	}
	Case m(SG_STACK_MEDIAN, SG_SIGMA, 64);	/* the rejection field of a MEDIAN stack does not count */
	CHECK(m.plan() == SG_OK && m.pl.redo == SG_REDO_SORTED && m.pl.replay_nm == 0);
}

static void test_route_addresses(void) {
	for (int method : {SG_STACK_MEAN, SG_STACK_MEDIAN}) {
		const int rej = method == SG_STACK_MEAN ? SG_SIGMA : SG_NO_REJEC;
		Case a(method, rej, 16, 32768, 16384);	/* H W 2 = 2^30 exactly */
		CHECK(a.plan(0, 4) == SG_OK && a.pl.main == SG_MAIN_HIST && a.pl.hist_addr_ok);
		Case b(method, rej, 16, 32768, 16385);
		CHECK(b.plan(0, 4) == SG_OK && b.pl.main == SG_MAIN_SORTED && !b.pl.hist_addr_ok);
	}
	for (int method : {SG_STACK_MEAN, SG_STACK_MEDIAN}) {
		const bool med = method == SG_STACK_MEDIAN;
		Case c(method, med ? SG_NO_REJEC : SG_SIGMA, 16, 64, 8);
		c.shifts();
		c.sx[3] = -16383;
		CHECK(c.plan() == SG_OK && c.pl.main == SG_MAIN_HIST && c.pl.hist_maxsx == (med ? 0 : 16383));
		c.sx[3] = 16384;
		CHECK(c.plan() == SG_OK && c.pl.main == (med ? SG_MAIN_HIST : SG_MAIN_SORTED));
		CHECK(c.pl.use_shift == (med ? 0 : 1));
		/* (H + |sy|) W 2 + 2 |sx| against 2^31 */
		Case e(method, med ? SG_NO_REJEC : SG_SIGMA, 16, 32768, 16384);
		e.shifts();
		e.sy[2] = 16383;
		e.sx[2] = 16383;
		CHECK(e.plan(0, 4) == SG_OK && e.pl.main == SG_MAIN_HIST);
		CHECK(med || (e.pl.sh[2] == 16383 * 65536 + 2 * 16383 && e.pl.sy_max == 16383 && e.pl.sy_min == 0));
		e.sy[2] = 16384;
		e.sx[2] = 0;
		CHECK(e.plan(0, 4) == SG_OK && e.pl.main == (med ? SG_MAIN_HIST : SG_MAIN_SORTED));
		CHECK(e.pl.sy_max == (med ? 0 : 16384));
	}
}

static void test_route_norm(void) {
	const int modes[5] = {SG_NO_NORM, SG_ADDITIVE, SG_MULTIPLICATIVE, SG_ADDITIVE_SCALING, SG_MULTIPLICATIVE_SCALING};
	const int folded[5] = {0, 3, 2, 3, 2}, plain[5] = {0, 1, 2, 1, 2};
	for (int i = 0; i < 5; i++) {
		Case c(SG_STACK_MEAN, SG_PERCENTILE, 16);
		c.norm(modes[i]);
		CHECK(c.plan() == SG_OK && c.pl.norm == folded[i] && c.pl.normalize == modes[i]);
		c.off[7] = 1e-30;
		CHECK(c.plan() == SG_OK && c.pl.norm == plain[i]);
		for (int method : {SG_STACK_SUM, SG_STACK_MAX, SG_STACK_MIN}) {
			Case r(method, SG_NO_REJEC, 16);
			r.norm(modes[i]);
			CHECK(r.plan() == SG_OK && r.pl.normalize == 0 && r.pl.nm.empty());
		}
	}
	/* 128-pixel tiles: W = 300 is 3 tiles a row, plain and normalised */
	for (int rej : {SG_SIGMA, SG_WINSORIZED, SG_PERCENTILE, SG_SIGMEDIAN}) {
		Case c(SG_STACK_MEAN, rej, 16, 300);
		CHECK(c.plan() == SG_OK && c.pl.main_grid[0] == 3 * 8);
		c.norm(SG_ADDITIVE);
		CHECK(c.plan() == SG_OK && c.pl.main_grid[0] == 3 * 8);
	}
	Case m(SG_STACK_MEDIAN, SG_NO_REJEC, 16, 300);
	CHECK(m.plan() == SG_OK && m.pl.main_grid[0] == 3 * 8);
	/* the staged verdict word and the load check */
	const unsigned int staged[3] = {3, 2, 0};
	for (int knob = 0; knob < 3; knob++)
		for (int mode : {SG_ADDITIVE, SG_MULTIPLICATIVE}) {
			Case c(SG_STACK_MEAN, SG_SIGMA, 20);
			c.norm(mode);
			c.k.norm_fma = knob;
			CHECK(c.plan() == SG_OK && c.pl.Npad == 32 && c.pl.nm.size() == (size_t)3 * 20 + 6 * 32 + 2);
			unsigned int w = 99;
			memcpy(&w, &c.pl.nm[3 * 20 + 4 * 32], sizeof w);
			CHECK(w == staged[knob] && c.pl.staged_verdict == staged[knob]);
			CHECK(c.pl.norm_check == (knob != 0));
			CHECK(c.pl.norm_fma == (knob == 0 ? 0 : (knob == 2 && mode == SG_ADDITIVE) ? 2 : 1));
		}
	Case u(SG_STACK_MEAN, SG_SIGMA, 20);
	CHECK(u.plan() == SG_OK && !u.pl.norm_check && u.pl.norm_fma == 0);
}

static void test_route_compact(void) {
	for (int rej : {SG_SIGMA, SG_WINSORIZED, SG_PERCENTILE, SG_SIGMEDIAN})
		for (int mode : {SG_NO_NORM, SG_ADDITIVE, SG_MULTIPLICATIVE}) {
			const bool on = (rej == SG_SIGMA || rej == SG_WINSORIZED) && mode != SG_NO_NORM;
			Case c(SG_STACK_MEAN, rej, 16);
			if (mode != SG_NO_NORM)
				c.norm(mode);
			CHECK(c.plan(2, 7) == SG_OK && c.pl.compact == on && c.pl.cmp_cap == (on ? (size_t)256 * 5 : 0));
			CHECK(c.pl.launches == (rej == SG_SIGMA || rej == SG_WINSORIZED ? 5 : 4) + (on ? 1 : 0));
			c.k.hist_compact = 5;
			CHECK(c.plan() == SG_OK && c.pl.compact == on && c.pl.cmp_cap == (on ? 5u : 0u));
			c.k.hist_compact = 0;
			CHECK(c.plan() == SG_OK && !c.pl.compact);
		}
	Case big(SG_STACK_MEAN, SG_SIGMA, 16, 4096, 4096);	/* 16.7 M pixels against 384 MiB / 32 B */
	big.norm(SG_ADDITIVE);
	CHECK(big.plan() == SG_OK && big.pl.compact && big.pl.cmp_cap == ((size_t)384 << 20) / 32);
	Case n(SG_STACK_MEAN, SG_SIGMA, 1025);
	n.norm(SG_ADDITIVE);
	CHECK(n.plan() == SG_OK && !n.pl.compact);
}

static void test_route_reduce(void) {
	const int methods[3] = {SG_STACK_SUM, SG_STACK_MAX, SG_STACK_MIN}, ms[3] = {0, 3, 4};
	for (int i = 0; i < 3; i++) {
		Case c(methods[i], SG_NO_REJEC, 8, 1000, 10, 3);
		CHECK(c.plan(2, 9) == SG_OK && c.pl.main == SG_MAIN_REDUCE3 && c.pl.m == ms[i] && c.pl.seg == 1);
		CHECK(c.pl.main_grid[0] == 2 * 7 * 3 && c.pl.main_grid[1] == 1 && c.pl.main_kernel_blocks == 42);
		CHECK(c.pl.launches == 1 && c.pl.path == 0 && c.pl.fin_grid_x == 4 && c.pl.sum == (i == 0) && c.pl.tables.empty());
		c.k.reduce_seg = 4;
		CHECK(c.plan(2, 9) == SG_OK && c.pl.seg == 4 && c.pl.main_grid[0] == 1 * 7 * 3);
		c.k.reduce1 = 2;
		CHECK(c.plan(2, 9) == SG_OK && c.pl.main == SG_MAIN_REDUCE2);
		CHECK(c.pl.main_grid[0] == 2 && c.pl.main_grid[1] == 7 && c.pl.main_grid[2] == 3 && c.pl.main_kernel_blocks == 42);
		c.k.reduce1 = 1;
		CHECK(c.plan(2, 9) == SG_OK && c.pl.main == SG_MAIN_REDUCE && c.pl.main_grid[0] == 4 && c.pl.main_kernel_blocks == 84);
	}
	Case m(SG_STACK_MEAN, SG_NO_REJEC, 8);
	CHECK(m.plan() == SG_OK && m.pl.main == SG_MAIN_REDUCE3 && m.pl.m == 1);
	m.norm(SG_MULTIPLICATIVE);
	CHECK(m.plan() == SG_OK && m.pl.m == 2 && m.pl.normalize == SG_MULTIPLICATIVE);
	Case w1(SG_STACK_SUM, SG_NO_REJEC, 8, 1, 8);
	CHECK(w1.plan() == SG_OK && w1.pl.main == SG_MAIN_REDUCE);
	Case w2(SG_STACK_SUM, SG_NO_REJEC, 8, 2, 8);
	CHECK(w2.plan() == SG_OK && w2.pl.main == SG_MAIN_REDUCE3);
	Case p31(SG_STACK_SUM, SG_NO_REJEC, 8, 32768, 32768);	/* W H 2 = 2^31: no pairs */
	CHECK(p31.plan(0, 2) == SG_OK && p31.pl.main == SG_MAIN_REDUCE);
	Case p30(SG_STACK_SUM, SG_NO_REJEC, 8, 32768, 16385);	/* pairs, but past the 2^30 plane offsets */
	CHECK(p30.plan(0, 2) == SG_OK && p30.pl.main == SG_MAIN_REDUCE2);
	Case sh(SG_STACK_MAX, SG_NO_REJEC, 8, 64, 8);
	sh.shifts();
	sh.sx[1] = 16384;
	CHECK(sh.plan() == SG_OK && sh.pl.main == SG_MAIN_REDUCE2 && sh.pl.use_shift == 1);
	/* N 65535 against the kernels' uint32_t sums: 65537 frames fit exactly and keep the route and the
	 * grid of any shorter stack, 65538 take the 64-bit kernel (SUM and MEAN, normalised or not; MAX
	 * and MIN add nothing up and stay) */
	CHECK(65537ull * 65535ull == 0xFFFFFFFFull && SG_SUM_U32_MAXN == 65537);
	for (int method : {SG_STACK_SUM, SG_STACK_MEAN, SG_STACK_MAX, SG_STACK_MIN})
		for (int mode : {SG_NO_NORM, SG_ADDITIVE_SCALING}) {
			const bool adds = method == SG_STACK_SUM || method == SG_STACK_MEAN;
			const int mm = method == SG_STACK_SUM ? 0 : method == SG_STACK_MAX ? 3 : method == SG_STACK_MIN ? 4 :
				mode == SG_NO_NORM ? 1 : 2;
			Case ref(method, SG_NO_REJEC, 8, 1000, 10, 3), fit(method, SG_NO_REJEC, 65537, 1000, 10, 3),
			     over(method, SG_NO_REJEC, 65538, 1000, 10, 3);
			for (Case *c : {&ref, &fit, &over}) {
				if (mode != SG_NO_NORM)
					c->norm(mode);
				CHECK(c->plan(2, 9) == SG_OK && c->pl.m == mm && c->pl.launches == 1 && c->pl.fin_grid_x == 4);
				CHECK(c->pl.main_threads == 256 && c->pl.sum == (method == SG_STACK_SUM));
			}
			CHECK(!ref.pl.wide && !fit.pl.wide && over.pl.wide == adds);
			CHECK(fit.pl.main == SG_MAIN_REDUCE3 && fit.pl.main == ref.pl.main && fit.pl.seg == ref.pl.seg);
			CHECK(fit.pl.main_grid[0] == 42 && fit.pl.main_grid[1] == 1 && fit.pl.main_grid[2] == 1);
			CHECK(fit.pl.main_kernel_blocks == 42 && ref.pl.main_kernel_blocks == 42);
			if (adds) {
				CHECK(over.pl.main == SG_MAIN_REDUCE_WIDE && over.pl.main_kernel_blocks == 84);
				CHECK(over.pl.main_grid[0] == 4 && over.pl.main_grid[1] == 7 && over.pl.main_grid[2] == 3);
			} else {
				CHECK(over.pl.main == SG_MAIN_REDUCE3 && over.pl.main_grid[0] == 42 && over.pl.main_kernel_blocks == 42);
			}
			/* the knobs that pick the narrow kernels do not bring the uint32_t sums back */
			over.k.reduce1 = 1;
			CHECK(over.plan(2, 9) == SG_OK && over.pl.main == (adds ? SG_MAIN_REDUCE_WIDE : SG_MAIN_REDUCE));
			fit.k.reduce1 = 1;
			CHECK(fit.plan(2, 9) == SG_OK && fit.pl.main == SG_MAIN_REDUCE && !fit.pl.wide);
		}
	Case rj(SG_STACK_MEAN, SG_SIGMA, 65538, 64, 4);	/* a rejection stack has no sums to widen */
	CHECK(rj.plan() == SG_OK && !rj.pl.wide && rj.pl.main == SG_MAIN_LITERAL_ALL);
}

static void test_errors(void) {
	Case a(SG_STACK_MEAN, SG_SIGMA, 1);
	CHECK(a.plan() == SG_ERR_GENERIC && !strcmp(a.pl.err, "select at least two frames (1)"));
	Case g(SG_STACK_MEAN, SG_SIGMA, 8);
	CHECK(g.plan(0, 9) == SG_ERR_SIZE && !strcmp(g.pl.err, "bad geometry 0"));
	CHECK(g.plan(3, 3) == SG_ERR_SIZE && g.plan(-1, 3) == SG_ERR_SIZE);
	g.d.nb_layers = 4;
	CHECK(g.plan() == SG_ERR_SIZE && !strcmp(g.pl.err, "bad geometry 0"));
	Case m(5, SG_SIGMA, 8);
	CHECK(m.plan() == SG_ERR_GENERIC && !strcmp(m.pl.err, "unknown method 5"));
	Case r(SG_STACK_MEAN, SG_SIGMA, 8);
	r.d.resident_rows[0] = 5;
	r.d.resident_rows[1] = 3;
	CHECK(r.plan() == SG_ERR_SIZE && !strcmp(r.pl.err, "bad resident row range 5"));
	r.d.resident_rows[0] = 2;
	r.d.resident_rows[1] = 6;
	CHECK(r.plan() == SG_ERR_SIZE &&
			!strcmp(r.pl.err, "frame rows 0..7 read by the band are not all resident (2..5)"));
	CHECK(r.plan(2, 6) == SG_OK && r.pl.res_begin == 2 && r.pl.res_end == 6);
	r.shifts();
	r.sy[1] = 1;
	CHECK(r.plan(2, 6) == SG_ERR_SIZE &&
			!strcmp(r.pl.err, "frame rows 1..5 read by the band are not all resident (2..5)"));
	/* tests/test_gpu_stack.py test_block_overflow_shift_refused */
	Case o(SG_STACK_MEAN, SG_SIGMA, 8, 64, 24);
	o.shifts();
	o.sy[3] = -9;
	CHECK(o.plan() == SG_ERR_GENERIC && !strcmp(o.pl.err, "a registration shift of -9 rows reaches above the block "
			"starting at row 6: the reference overflows its block buffer there (stacking.c:1555-1561); use more rows "
			"per block (max_number_of_rows / fewer threads)"));
	o.d.rejection = SG_NO_REJEC;
	CHECK(o.plan() == SG_ERR_GENERIC && strstr(o.pl.err, "overflows"));
	o.d.rejection = SG_SIGMA;
	o.sy[3] = -5;
	CHECK(o.plan() == SG_OK && o.pl.nblocks == 4 && o.pl.sy_min == -5);
}

static void test_params(void) {
	Case c(SG_STACK_MEAN, SG_WINSORIZED, 20, 300, 9, 3);
	c.shifts();
	c.sy[4] = 2;
	c.sx[4] = -7;
	c.k.hist_dbg = 5;
	c.k.hist_prio = 2;
	c.k.wins_cap = 17;
	CHECK(c.plan(1, 8) == SG_OK);
	SgStackParams p;
	sg_plan_params(c.pl, p);
	CHECK(p.N == 20 && p.W == 300 && p.H == 9 && p.C == 3 && p.method == SG_STACK_MEAN && p.rejection == SG_WINSORIZED);
	CHECK(p.sig0 == 4.0 && p.sig1 == 3.0 && p.use_shift == 1 && p.row_begin == 1 && p.row_end == 8);
	CHECK(p.res_begin == 0 && p.res_end == 9 && p.sy_min == 0 && p.sy_max == 2 && p.hist_maxsx == 7 && p.hist_npad == 32);
	CHECK(p.dbg == 5 && p.prio == 2 && p.wins_cap == 17 && !p.frames && !p.out && !p.flag_count);
	/* the shift table: c1, sx2, shiftx, shifty */
	CHECK(c.pl.sh.size() == 32 + 16 + 40 && c.pl.sh[4] == 2 * 300 * 2 - 14 && ((int16_t *)&c.pl.sh[32])[4] == -14);
	CHECK(c.pl.sh[48 + 4] == -7 && c.pl.sh[48 + 20 + 4] == 2);
}

/* the knobs of the removed A/B paths (256-pixel tiles, exported Winsorize columns, LINEARFIT
 * lockstep pairs) are no longer read: with them set, the plans equal those of a clean environment.
 * same_plan lists the route and launch fields by hand: a field added to SgStackPlan belongs here too */
static bool same_plan(const SgStackPlan &a, const SgStackPlan &b) {
	return a.main == b.main && a.rj == b.rj && a.norm == b.norm && a.nreg == b.nreg && a.km == b.km && a.nw == b.nw &&
		a.main_grid[0] == b.main_grid[0] && a.main_grid[1] == b.main_grid[1] && a.main_grid[2] == b.main_grid[2] &&
		a.main_threads == b.main_threads && a.main_lds == b.main_lds && a.sorted_lds == b.sorted_lds &&
		a.launches == b.launches && a.main_kernel_blocks == b.main_kernel_blocks && a.path == b.path &&
		a.compact == b.compact && a.cmp_cap == b.cmp_cap && a.redo == b.redo && a.rp_maxn == b.rp_maxn &&
		a.list_minn == b.list_minn && a.replay_nm == b.replay_nm && a.linfit_tables == b.linfit_tables &&
		a.norm_check == b.norm_check && a.scratch_bytes == b.scratch_bytes && a.npix_launch == b.npix_launch &&
		a.sh == b.sh && a.nm == b.nm && a.tables == b.tables && a.ztab == b.ztab;
}
static void test_removed_knobs(void) {
	const char *names[3] = {"SG_HIST_NI", "SG_WINS_EXPORT", "SG_LINFIT_PAIR"};
	const int rej[3] = {SG_SIGMA, SG_WINSORIZED, SG_LINEARFIT};
	for (int i = 0; i < 3; i++) {
		for (const char *n : names)
			unsetenv(n);
		Case clean(SG_STACK_MEAN, rej[i], 16, 300);
		clean.k.read();
		CHECK(clean.plan() == SG_OK);
		setenv("SG_HIST_NI", "2", 1);
		setenv("SG_WINS_EXPORT", "1", 1);
		setenv("SG_LINFIT_PAIR", "1", 1);
		Case set(SG_STACK_MEAN, rej[i], 16, 300);
		set.k.read();
		CHECK(set.plan() == SG_OK);
		CHECK(same_plan(clean.pl, set.pl));
		CHECK(set.pl.main == (rej[i] == SG_LINEARFIT ? SG_MAIN_LINFIT : SG_MAIN_HIST));
		CHECK(set.pl.main_grid[0] == (rej[i] == SG_LINEARFIT ? 5u * 8 : 3u * 8));
	}
	for (const char *n : names)
		unsetenv(n);
}

int main(int argc, char **argv) {
	test_removed_knobs();
	test_chain_tables();
	test_additive_fold(argc > 1 ? atoi(argv[1]) : 200);
	test_ztab();
	test_route_n15_n16();
	test_route_linfit();
	test_route_large_n();
	test_route_replay();
	test_route_addresses();
	test_route_norm();
	test_route_compact();
	test_route_reduce();
	test_errors();
	test_params();
	printf("checks=%d bad=%d\n", checks, bad);
	return bad != 0;
}
'''


FOLD_SETS = 200
FOLD_SETS_SANITIZED = 40


def _build(tmp_path, extra, opt="-O1"):
    src = tmp_path / "stack_plan_check.cpp"
    src.write_text(PROGRAM)
    exe = tmp_path / "stack_plan_check"
    objs = []
    for name in ("or_stacking", "or_core"):
        obj = tmp_path / (name + ".o")
        r = subprocess.run(["gcc", *ORC_CFLAGS, *extra, "-I", ORC, "-c", os.path.join(ORC, name + ".c"), "-o", str(obj)],
                           capture_output=True, text=True)
        if r.returncode != 0:
            return exe, r
        objs.append(str(obj))
    r = subprocess.run(["g++", opt, "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-D__HIP_PLATFORM_AMD__", *extra,
                        "-I", INC, "-I", ORC, "-I", ROCM_INC, str(src), *objs, "-o", str(exe), "-fopenmp", "-lm"],
                       capture_output=True, text=True)
    return exe, r


def _run(exe, fold_sets):
    r = subprocess.run([str(exe), str(fold_sets)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    assert " bad=0" in r.stdout and "checks=" in r.stdout, r.stdout[-2000:]


def test_stack_plan_matches_oracle_and_known_routes(tmp_path):
    exe, r = _build(tmp_path, [])
    assert r.returncode == 0, r.stderr[-4000:]
    _run(exe, FOLD_SETS)


def test_stack_plan_sanitized(tmp_path):
    """the same program under AddressSanitizer + UBSan (host code only, run stand-alone)"""
    # the runtimes are linked statically: the program then runs whatever else the loader brings in
    san = ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan"]
    probe = tmp_path / "probe.c"
    probe.write_text("int main(void) { return 0; }\n")
    p = subprocess.run(["gcc", *san, str(probe), "-o", str(tmp_path / "probe")], capture_output=True, text=True)
    if p.returncode != 0 or subprocess.run([str(tmp_path / "probe")]).returncode != 0:
        pytest.skip("the AddressSanitizer / UBSan runtime is not installed")
    exe, r = _build(tmp_path, san, "-O0")      # unoptimised: the instrumented build is most of this test's time
    assert r.returncode == 0, r.stderr[-4000:]
    _run(exe, FOLD_SETS_SANITIZED)
