/*
 * sg_reg_plan.hpp - the host-only half of a DFT registration call: from the frame count, the
 * side, the reference, the mask and the knobs to everything the launch steps (sg_register.hip,
 * reg_dft_device) need to know.
 *
 * sg_reg_plan() checks the arguments, lists the frames and the pairs, decides the route (generic
 * mixed-radix / Bluestein, fp64 or fp32 half spectra, block- or wave-level fp32 passes), every
 * thread count, LDS size, strip width and batch count, the quality route, the byte layouts of
 * the tables, the workspace and the pinned block, and the kernels whose dynamic LDS limit the
 * call raises.  The table builders (twiddles, the mixed-radix plan, Bluestein's chirp and its
 * spectrum) live here too.  Nothing here calls a HIP function, takes a device pointer or reads
 * the environment, so a plain host program can call it (tests/test_reg_plan_cpu.py).
 */
#pragma once
#include <math.h>
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <algorithm>
#include <vector>
#include "sg_common.hpp"
#include "sg_ctx.hpp"

/* ---- plain data shared with the kernels (sg_fft.hpp, sg_register.hip) ---- */
#define SG_PADN(n) ((n) + ((n) >> 3))
/* element stride between the columns of a column-strip kernel (k_reg_cols, k_reg_cols_xpower):
 * float2 strips +4 so that the batch-minor passes (4 columns x 8 consecutive elements per 32-lane
 * group: the last FFT pass, the cross power, the inverse's first pass) and the first pass's
 * stores fall on distinct banks -- a bank model of the S = 2048 pass (64 banks for ds_read_b64,
 * 32 for ds_write_b64, MI355X_MICROARCH.md LDS) gives 1.54x the conflict-free LDS cycles against
 * 2.62x at +1, and SQ_LDS_BANK_CONFLICT of the pass was 2.05x its active LDS cycles
 * (profiles/r04r_sq_register_1.txt); double2 strips keep +1 */
template <class C>
__host__ __device__ constexpr int sg_col_stride(int S) {
	return SG_PADN(S) + (sizeof(C) == 8 ? 4 : 1);
}

#define SG_WCOL_CS 2120	/* LDS float2 per column: 2048 (strip) / 32 x 66 (transposes), +8 for the strip's banks */

#define SG_GEN_MAXPASS 16
struct SgGenPlan {
	int n, npass;
	int radix[SG_GEN_MAXPASS];
	int bluestein, m;	/* Bluestein: convolution length m (power of two) */
};

#define SG_CAND_CAP 64

/* sizes of the device structs the layouts count in (SgBest, SgCand: sg_fft.hpp; SgRegOut:
 * sg_register.hip, which pins each against its struct) and of the two complex element types */
#define SG_REG_SIZEOF_BEST 48
#define SG_REG_SIZEOF_OUT 80
#define SG_REG_SIZEOF_CAND 776
#define SG_REG_SIZEOF_C64 16
#define SG_REG_SIZEOF_C32 8

/* ---- host table builders ---- */

/* forward full circle exp(-2 pi i k / n), k < n, then its conjugate (the inverse), as the
 * device transforms read them (sg_twiddle).  Power of two: the half circle, negated exactly
 * for k >= n/2; otherwise every k directly. */
static void make_twiddles(int n, std::vector<double> &tw) {
	tw.assign(4 * (size_t)n, 0.0);
	const bool pow2 = (n & (n - 1)) == 0;
	for (int k = 0; k < (pow2 ? n / 2 : n); k++) {
		const double a = -2.0 * M_PI * (double)k / (double)n;
		const double c = cos(a), sn = sin(a);
		const int nk = pow2 ? 2 : 1;
		const int kk[2] = {k, k + n / 2};
		const double sg[2] = {1.0, -1.0};
		for (int h = 0; h < nk; h++) {
			tw[2 * kk[h]] = sg[h] * c;
			tw[2 * kk[h] + 1] = sg[h] * sn;
			tw[2 * (n + kk[h])] = sg[h] * c;
			tw[2 * (n + kk[h]) + 1] = -(sg[h] * sn);
		}
	}
}

/* the fp32 twiddles: the fp64 table, each value rounded */
static void make_twiddles32(int n, std::vector<float> &t32) {
	std::vector<double> t64;
	make_twiddles(n, t64);
	t32.resize(t64.size());
	for (size_t i = 0; i < t64.size(); i++)
		t32[i] = (float)t64[i];
}

/* radices of an n-point mixed-radix plan (8, 4, 2, 3, 5, 7); false: a prime factor > 7 */
static bool make_plan(int n, SgGenPlan &pl) {
	memset(&pl, 0, sizeof pl);
	pl.n = n;
	int r = n;
	const int rad[6] = {8, 4, 2, 3, 5, 7};
	for (int q = 0; q < 6; q++)
		while (r % rad[q] == 0 && pl.npass < SG_GEN_MAXPASS) {
			pl.radix[pl.npass++] = rad[q];
			r /= rad[q];
		}
	return r == 1;
}

/* in-place radix-2 complex DFT on the host (Bluestein's chirp spectrum, computed once per call) */
static void host_fft_pow2(std::vector<double> &re, std::vector<double> &im, int n) {
	for (int i = 1, j = 0; i < n; i++) {
		int bit = n >> 1;
		for (; j & bit; bit >>= 1)
			j ^= bit;
		j ^= bit;
		if (i < j) {
			std::swap(re[i], re[j]);
			std::swap(im[i], im[j]);
		}
	}
	for (int len = 2; len <= n; len <<= 1) {
		for (int i = 0; i < n; i += len)
			for (int k = 0; k < len / 2; k++) {
				const double a = -2.0 * M_PI * (double)k / (double)len;
				const double wr = cos(a), wi = sin(a);
				const double xr = re[i + k + len / 2], xi = im[i + k + len / 2];
				const double vr = xr * wr - xi * wi, vi = xr * wi + xi * wr;
				re[i + k + len / 2] = re[i + k] - vr;
				im[i + k + len / 2] = im[i + k] - vi;
				re[i + k] += vr;
				im[i + k] += vi;
			}
	}
}

/* Bluestein's tables of an S-point transform through an m-point convolution: the chirp
 * c_j = exp(-i pi j^2 / S), j < S, and bhat = FFT_m(b), b_j = b_{m-j} = conj c_j */
static void make_bluestein(int S, size_t m, std::vector<double> &ch, std::vector<double> &bh) {
	ch.assign(2 * (size_t)S, 0.0);
	std::vector<double> br(m, 0.0), bi(m, 0.0);
	for (int j = 0; j < S; j++) {
		const long long q = ((long long)j * j) % (2ll * S);	/* j^2 mod 2S keeps the angle exact */
		const double a = -M_PI * (double)q / (double)S;
		ch[2 * j] = cos(a);
		ch[2 * j + 1] = sin(a);
		br[j] = ch[2 * j];
		bi[j] = -ch[2 * j + 1];	/* b_j = conj c_j */
		if (j) {
			br[m - j] = br[j];
			bi[m - j] = bi[j];
		}
	}
	host_fft_pow2(br, bi, (int)m);
	bh.assign(2 * m, 0.0);
	for (size_t k = 0; k < m; k++) {
		bh[2 * k] = br[k];
		bh[2 * k + 1] = bi[k];
	}
}

static int ilog2(int v) {
	int l = 0;
	while ((1 << l) < v)
		l++;
	return l;
}

/* ---- the plan ---- */

/* the passes of a call */
enum SgRegRoute {
	SG_REG_GEN_MIXED = 0,	/* any side: mixed radix 8/4/2/3/5/7 rows, transposed columns, fp64 */
	SG_REG_GEN_BLUESTEIN,	/* a prime factor above 7: chirp-z rows */
	SG_REG_HALF64,		/* power of two: half-spectrum passes in fp64 */
	SG_REG_HALF32_BLOCK,	/* ... in fp32, block-level passes; near ties re-run in fp64 */
	SG_REG_HALF32_WAVE	/* ... in fp32, the wave-level passes of S = 2048 */
};
/* the fused fp32 column pass (forward columns, cross power, inverse columns) */
enum SgRegCols32 {
	SG_COLS32_BLOCK8_OCC = 0,	/* k_reg_cols_xpower<float2, 8, 8>: 64 VGPRs (8 waves / SIMD, two 1024-thread workgroups per CU) */
	SG_COLS32_BLOCK16,		/* k_reg_cols_xpower<float2, 16>: 16 elements per thread */
	SG_COLS32_WAVE8_PERM		/* k_reg_cols_xpower_w: 8-column strips, 64-B row segments, one workgroup per CU, the reference spectrum in lane order */
};
/* when the quality estimate is queued */
enum SgRegQRoute {
	SG_REG_Q_FOLDED = 0,	/* the subsample inside the wave-level forward rows, the gradient behind the last batch's */
	SG_REG_Q_UPFRONT	/* ahead of the reference spectrum */
};
/* the kernels with dynamic LDS */
enum SgRegKernel {
	SG_RK_GEN_COLS_XPOWER = 0,
	SG_RK_GEN_ROWS_BLUE,		/* k_gen_rows<true> */
	SG_RK_GEN_ROWS,			/* k_gen_rows<false> */
	SG_RK_COLS64,			/* k_reg_cols<sg_c64, 8> */
	SG_RK_FWD64,			/* k_reg_rows_fwd_half<sg_c64> */
	SG_RK_INV64,			/* + candidates: k_reg_rows_inv_half_argmax<sg_c64, false / true> */
	SG_RK_INV64_CAND,
	SG_RK_XPOWER64,			/* k_reg_cols_xpower<sg_c64, 8> */
	SG_RK_FWD32,			/* k_reg_rows_fwd_half<float2> */
	SG_RK_INV32,			/* k_reg_rows_inv_half_argmax<float2, false> */
	SG_RK_COLS32_8,			/* + (ept32 == 16): k_reg_cols<float2, 8 / 16> */
	SG_RK_COLS32_16,
	SG_RK_XPOWER32,			/* + SgRegCols32: the three instances of the fused column pass */
	SG_RK_XPOWER32_END = SG_RK_XPOWER32 + 3,
	SG_RK_FWD_PERM_W = SG_RK_XPOWER32_END,	/* k_reg_cols_fwd_perm_w */
	SG_RK_FWD_W,			/* + folded: k_reg_rows_fwd_half_w<false / true> */
	SG_RK_FWD_W_FOLD,
	SG_RK_INV_W,			/* k_reg_rows_inv_half_w */
	SG_RK_COUNT
};
struct SgRegLdsAttr {
	int kernel;	/* SgRegKernel */
	int bytes;
};

struct SgRegPlan {
	char err[512];			/* the message of a failed plan (sg_last_error's text) */
	int nframes, S, ref_image;	/* ref_image: -1 planned as 0 */
	int64_t fpitch, rpitch;		/* selection f row r at f fpitch + r rpitch (elements) */
	/* frames to register in index order; the quality estimate's frames (the reference, then todo);
	 * pair k = frames hfa[k], hfb[k] (-1: odd count, imaginary part zero), slot NP the reference
	 * spectrum's (ref_image, -1) */
	std::vector<int> todo, qframes, hfa, hfb;
	int npairs_total, NP;
	/* the route */
	int route;			/* SgRegRoute */
	bool generic, fp32, wcol;	/* wcol: S = 2048 and the knob (the wave-level passes when fp32) */
	SgGenPlan gen;
	int gen_thr;
	size_t gen_lds;
	bool gen_fuse;
	/* pass sizes */
	size_t plane, esz, pair_bytes;
	int B, Bc, B64;			/* pairs per launch: the knob or the 2 GB rule, at least 1, the fp64 re-runs */
	int row_thr;
	size_t row_lds, row_lds32;
	int CW, CWh, colh_thr;
	size_t colh_lds;
	int CW32, ept32, colh_thr32;
	size_t colh_lds32, wcol_lds;
	int rpw, rpb, logS, tol_main;
	unsigned int tgrid;		/* k_gen_transpose: (tgrid, tgrid, pairs) */
	/* knob-derived switches */
	int cols32;			/* SgRegCols32 */
	int qroute, qfold;		/* SgRegQRoute; rows per wave of the folded subsample (0: not folded) */
	bool specp_on;			/* the fp32 reference spectrum also in the wave-level column pass's lane order */
	/* byte layouts: reg_tw in doubles (tw, then for Bluestein twm, the chirp, bhat) */
	size_t n_tw, n_twm, n_ch, n_bh, tab_total;
	size_t spec_bytes, work_bytes;
	size_t o_out, o_fab, o_en, o_cand, o_res2, ws;
	size_t pin_res, pin_bytes;
	std::vector<SgRegLdsAttr> lds_attrs;	/* raised with hipFuncSetAttribute, in this order */
};

static int sg_reg_plan_fail(SgRegPlan &pl, int code, const char *fmt, ...) {
	va_list ap;
	va_start(ap, fmt);
	vsnprintf(pl.err, sizeof pl.err, fmt, ap);
	va_end(ap);
	return code;
}

static size_t sg_align256(size_t v) {
	return (v + 255) & ~(size_t)255;
}

/* frames to register, the quality estimate's list and the pair table */
static void sg_reg_plan_frames(const int *included, SgRegPlan &pl) {
	/* frames to register, in index order (the reference skips ref and excluded frames) */
	for (int f = 0; f < pl.nframes; f++)
		if (f != pl.ref_image && (!included || included[f]))
			pl.todo.push_back(f);
	/* quality of the reference and of every registered frame */
	pl.qframes.push_back(pl.ref_image);
	pl.qframes.insert(pl.qframes.end(), pl.todo.begin(), pl.todo.end());
	pl.npairs_total = (int)(pl.todo.size() + 1) / 2;
	const int NP = pl.NP = pl.npairs_total > 0 ? pl.npairs_total : 1;
	pl.hfa.assign(NP + 1, 0);
	pl.hfb.assign(NP + 1, 0);
	for (int k = 0; k < pl.npairs_total; k++) {
		pl.hfa[k] = pl.todo[2 * k];
		pl.hfb[k] = (2 * (size_t)k + 1 < pl.todo.size()) ? pl.todo[2 * k + 1] : -1;
	}
	pl.hfa[NP] = pl.ref_image;
	pl.hfb[NP] = -1;
}

/* the generic route: its transform plan, the row kernel's threads and LDS, the fused columns */
static void sg_reg_plan_generic(const SgKnobs &k, SgRegPlan &pl) {
	const int S = pl.S;
	SgGenPlan &g = pl.gen;
	if (!make_plan(S, g)) {
		g.bluestein = 1;
		g.m = 1;
		while (g.m < 2 * S - 1)
			g.m <<= 1;
	}
	pl.route = g.bluestein ? SG_REG_GEN_BLUESTEIN : SG_REG_GEN_MIXED;
	/* generic rows: Bluestein needs m/8 threads (sg_lds_fft), the mixed passes ceil(S / 8) (ceil(S / 7)
	 * with a radix-7 pass) rounded to whole waves (sg_gen_pass_ip's items per thread) */
	bool has7 = false;
	for (int q = 0; q < g.npass; q++)
		has7 |= g.radix[q] == 7;
	pl.gen_thr = g.bluestein ? (g.m / 8 < 64 ? 64 : g.m / 8)
				 : std::max(64, ((has7 ? (S + 6) / 7 : (S + 7) / 8) + 63) / 64 * 64);
	pl.gen_lds = g.bluestein ? (size_t)SG_PADN(g.m) * SG_REG_SIZEOF_C64 : pl.row_lds;
	/* the fused generic column pass: mixed-radix plans whose two rows fit a block and the LDS
	 * (SG_REG_GENFUSE=0: the three-kernel sequence, A/B) */
	pl.gen_fuse = !g.bluestein && 2 * pl.gen_thr <= 1024 && 2 * pl.gen_lds <= 160 * 1024 && k.reg_genfuse;
	if (pl.gen_fuse)
		pl.lds_attrs.push_back({SG_RK_GEN_COLS_XPOWER, (int)(2 * pl.gen_lds)});
	/* one instantiation per transform kind (register allocation is per kernel) */
	pl.lds_attrs.push_back({g.bluestein ? SG_RK_GEN_ROWS_BLUE : SG_RK_GEN_ROWS, (int)pl.gen_lds});
}

/* the half-spectrum routes of a power of two: strips, threads and LDS of the fp64 and the fp32
 * passes (an fp32 call re-runs its near ties through the fp64 ones) */
static void sg_reg_plan_half(const SgKnobs &k, SgRegPlan &pl) {
	const int S = pl.S;
	pl.wcol = S == 2048 && k.reg_wcol;	/* the wave-level fp32 column pass: S = 2048 only (32 x 64 four-step transforms) */
	pl.route = !pl.fp32 ? SG_REG_HALF64 : pl.wcol ? SG_REG_HALF32_WAVE : SG_REG_HALF32_BLOCK;
	int CW = 8192 / S;
	if (CW < 1)
		CW = 1;
	if (CW > 8)
		CW = 8;
	if (k.reg_cw > 0)	/* A/B knob SG_REG_CW: columns per column-pass workgroup */
		CW = k.reg_cw;
	pl.CW = CW;
	/* threads: 8 elements per thread in every fp64 LDS FFT (sg_stockham_pass's register
	 * budget), 16 in the fp32 column pass; at least one wave, at most 1024 */
	auto thr_for = [](int elems) { return elems / 8 < 64 ? 64 : elems / 8; };
	pl.row_thr = thr_for(S);
	/* half-spectrum columns: a strip stays inside one half (CW divides S/2) */
	pl.CWh = CW < S / 2 ? CW : S / 2;
	pl.colh_lds = (size_t)pl.CWh * sg_col_stride<double2>(S) * SG_REG_SIZEOF_C64;
	pl.colh_thr = thr_for(pl.CWh * S);
	/* fp32 columns: CW32 columns per strip (8: 64-B row segments), 16 elements per thread */
	int CW32 = k.reg_cw32;
	while (CW32 > 1 && (CW32 > S / 2 || CW32 * S > 16 * 1024))
		CW32 >>= 1;
	pl.CW32 = CW32;
	pl.ept32 = CW32 * S / 1024 > 8 ? 16 : 8;
	pl.colh_thr32 = std::max(64, CW32 * S / pl.ept32);
	pl.colh_lds32 = (size_t)CW32 * sg_col_stride<float2>(S) * SG_REG_SIZEOF_C32;
	int rpw = k.reg_rpw;	/* A/B knob SG_REG_RPW: rows per wave of the wave-level forward rows */
	while (rpw > 1 && (S / 4) % rpw)
		rpw >>= 1;
	pl.rpw = rpw;
	pl.wcol_lds = (size_t)4 * SG_WCOL_CS * SG_REG_SIZEOF_C32;
	/* rows per forward-row workgroup (the next row prefetched during this one's transform) */
	int rpb = k.reg_rpb;
	while (rpb > 1 && S % rpb != 0)
		rpb >>= 1;
	pl.rpb = rpb;
	/* wave-level column pass: the fp32 reference spectrum also in its lane order (k_reg_cols_fwd_perm_w) */
	pl.specp_on = pl.fp32 && pl.wcol;
	pl.cols32 = pl.wcol ? SG_COLS32_WAVE8_PERM : pl.ept32 == 16 ? SG_COLS32_BLOCK16 : SG_COLS32_BLOCK8_OCC;
	const int row = (int)pl.row_lds, row32 = (int)pl.row_lds32, col = (int)pl.colh_lds, col32 = (int)pl.colh_lds32,
		  w = (int)pl.wcol_lds;
	pl.lds_attrs = {{SG_RK_COLS64, col}, {SG_RK_FWD64, row}, {SG_RK_INV64, row}, {SG_RK_INV64_CAND, row},
		{SG_RK_XPOWER64, col}, {SG_RK_FWD32, row32}, {SG_RK_INV32, row32}, {SG_RK_COLS32_8, col32},
		{SG_RK_COLS32_16, col32}, {SG_RK_XPOWER32 + SG_COLS32_BLOCK8_OCC, col32},
		{SG_RK_XPOWER32 + SG_COLS32_BLOCK16, col32}, {SG_RK_XPOWER32 + SG_COLS32_WAVE8_PERM, 2 * w},
		{SG_RK_FWD_PERM_W, w}, {SG_RK_FWD_W, w}, {SG_RK_FWD_W_FOLD, w}, {SG_RK_INV_W, w}};
}

/* pairs per launch and the quality route */
static void sg_reg_plan_batches(const SgKnobs &k, SgRegPlan &pl) {
	const int S = pl.S;
	/* pairs per launch: up to 2 GB of pair planes (32 at S = 2048 on the fp64 half path).
	 * Half-spectrum passes, configs[1]: 32 or 64 pairs 8.95-9.07 ms, 16: 9.08, 4: 9.22-9.32,
	 * 2: 9.02-9.15, 1: 9.8 ms of registration (round-2 gpu_regbatch.sh) */
	pl.pair_bytes = pl.plane * pl.esz * (pl.generic ? 2 : 1);	/* generic: + transposed plane */
	int B = (int)((size_t)(2048u << 20) / pl.pair_bytes);
	if (B < 1)
		B = 1;
	if (B > 64)
		B = 64;
	if (k.reg_batch > 0)	/* A/B knob SG_REG_BATCH: pairs per launch */
		B = k.reg_batch;
	if (B > pl.npairs_total && pl.npairs_total > 0)
		B = pl.npairs_total;
	pl.B = B;
	pl.Bc = B > 1 ? B : 1;
	/* fp64 re-runs of near ties in the same work buffer */
	pl.B64 = pl.fp32 ? (int)std::max<size_t>(1, (size_t)pl.Bc * pl.pair_bytes / (pl.plane * SG_REG_SIZEOF_C64)) : pl.Bc;
	/* SG_REG_QFOLD (A/B): the quality estimate's subsample from the wave-level forward rows (every
	 * frame of qframes passes through them: the reference and each pair), then only the gradient
	 * kernel on the aux stream behind the last batch's forward rows */
	pl.qfold = (pl.specp_on && pl.npairs_total > 0 && S == 2048) ? k.reg_qfold : 0;
	pl.qroute = pl.qfold ? SG_REG_Q_FOLDED : SG_REG_Q_UPFRONT;
	pl.tol_main = pl.fp32 ? -15 : -32;
}

/* byte layouts: the tables of reg_tw, reg_spec, reg_work, the workspace and the pinned block */
static void sg_reg_plan_layout(SgRegPlan &pl) {
	const int S = pl.S, NP = pl.NP;
	const size_t plane = pl.plane;
	const bool blue = pl.gen.bluestein != 0;
	const size_t m = blue ? (size_t)pl.gen.m : 1;
	/* table layout: tw (4 S), then for Bluestein twm (4 m), the chirp (2 S), bhat (2 m) */
	pl.n_tw = 4 * (size_t)S;
	pl.n_twm = blue ? 4 * m : 0;
	pl.n_ch = blue ? 2 * (size_t)S : 0;
	pl.n_bh = blue ? 2 * m : 0;
	pl.tab_total = pl.n_tw + pl.n_twm + pl.n_ch + pl.n_bh;
	/* device workspace: reference spectrum (fp64, and fp32 behind it), pair planes, per-row
	 * partials, then (all pairs of the call, uploaded once / read back once) the pair table,
	 * the per-pair results, the frames' energies (two sets: the main passes and the near-tie
	 * re-runs) and the near-tie candidates of one batch */
	pl.spec_bytes = plane * SG_REG_SIZEOF_C64 + (pl.fp32 ? plane * SG_REG_SIZEOF_C32 : 0) +
			(pl.specp_on ? plane / 2 * SG_REG_SIZEOF_C32 : 0);
	/* the fp64 near-tie re-runs use the same buffer: at least one fp64 plane (B64 >= 1 even
	 * when the fp32 batch is a single pair, whose plane is half that size) */
	pl.work_bytes = std::max((size_t)pl.Bc * pl.pair_bytes, (size_t)pl.B64 * plane * SG_REG_SIZEOF_C64);
	pl.o_out = sg_align256((size_t)std::max(pl.Bc, pl.B64) * S * SG_REG_SIZEOF_BEST);
	pl.o_fab = pl.o_out + sg_align256((size_t)(NP + 1) * SG_REG_SIZEOF_OUT);
	pl.o_en = pl.o_fab + sg_align256((size_t)(NP + 1) * 4 * sizeof(int));
	pl.o_cand = pl.o_en + sg_align256((size_t)pl.nframes * 2 * sizeof(unsigned long long));
	pl.o_res2 = pl.o_cand + sg_align256((size_t)std::max(pl.Bc, pl.B64) * 2 * SG_REG_SIZEOF_CAND);
	pl.ws = pl.o_res2 + (size_t)(NP + 1) * SG_REG_SIZEOF_OUT;
	/* the pair table goes up, and the results come back, through a pinned block */
	pl.pin_res = ((size_t)2 * (NP + 1) * sizeof(int) + 63) & ~(size_t)63;
	pl.pin_bytes = pl.pin_res + (size_t)NP * SG_REG_SIZEOF_OUT;
}

/*
 * plan the registration of nframes selections of side S against frame ref_image under the knobs
 * k.  SG_OK, or the call's return code with its message in pl.err; a failed plan is not launched.
 */
static int sg_reg_plan(int nframes, int S, int ref_image, const int *included, int64_t fpitch, int64_t rpitch,
		const SgKnobs &k, SgRegPlan &pl) {
	pl = SgRegPlan();	/* every field zero, the lists empty */
	if (nframes < 1)
		return sg_reg_plan_fail(pl, SG_ERR_GENERIC, "no frame to register%s%ld", "", (long)nframes);
	if (S < 4 || S > 4096)
		return sg_reg_plan_fail(pl, SG_ERR_SIZE, "DFT registration takes selection sides 4 to 4096%s (got %ld)", "", (long)S);
	if (ref_image < 0)
		ref_image = 0;	/* seq->reference_image == -1 -> 0 (:212-215) */
	if (ref_image >= nframes)
		return sg_reg_plan_fail(pl, SG_ERR_GENERIC, "reference image out of range%s %ld", "", (long)ref_image);
	pl.nframes = nframes;
	pl.S = S;
	pl.ref_image = ref_image;
	pl.fpitch = fpitch;
	pl.rpitch = rpitch;
	pl.logS = ilog2(S);
	pl.plane = (size_t)S * S;
	pl.tgrid = (unsigned)((S + 31) / 32);
	sg_reg_plan_frames(included, pl);
	/* power-of-two sides take the half-spectrum passes; any other side the generic mixed-radix /
	 * Bluestein passes (SG_REG_PATH=3 forces those for a power of two, A/B; the round-1/2 full-
	 * spectrum pass orders 0 / 1 were removed in round 4) */
	pl.generic = (S & (S - 1)) != 0 || S < 8 || k.reg_path == 3;
	/* precision of the main passes: the power-of-two half-spectrum passes run in fp32
	 * (SG_REG_FP=32, default: half the plane bytes and LDS), and a pair whose correlation
	 * maximum is a near tie at fp32 tolerance is re-run in fp64 (the arg-max is then exactly
	 * the fp64 one wherever fp64 is not itself near a tie; those go to the exact integer
	 * correlations).  The other pass orders and the generic path are fp64. */
	pl.fp32 = !pl.generic && k.reg_fp == 32;
	pl.esz = pl.fp32 ? SG_REG_SIZEOF_C32 : SG_REG_SIZEOF_C64;
	pl.row_lds = (size_t)SG_PADN(S) * SG_REG_SIZEOF_C64;
	pl.row_lds32 = (size_t)SG_PADN(S) * SG_REG_SIZEOF_C32;
	if (pl.generic)
		sg_reg_plan_generic(k, pl);
	else
		sg_reg_plan_half(k, pl);
	sg_reg_plan_batches(k, pl);
	sg_reg_plan_layout(pl);
	return SG_OK;
}
