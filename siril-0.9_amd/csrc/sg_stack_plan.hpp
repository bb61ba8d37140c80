/*
 * sg_stack_plan.hpp - the host-only half of a stacking call: from the descriptor, the row band
 * and the knobs to everything the launch step (sg_api.cpp, stack_device_core) needs to know.
 *
 * sg_stack_plan() checks the arguments, builds the four host tables the kernels read (shift
 * table, normalisation table, border-row table, chain tables) and decides the route: which main
 * kernel with which template arguments, how its redo pixels travel, every grid and LDS size and
 * the statistics that follow from them.  It calls no HIP function, takes no device pointer and
 * reads no environment, so a plain host program can call it (tests/test_stack_plan_cpu.py).
 */
#pragma once
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <unistd.h>
#include <algorithm>
#include <vector>
#include "sg_common.hpp"
#include "sg_ctx.hpp"

/* blocks of the listed k_stack_sorted launches (grid-stride over any list length) */
#define SG_LIST_GRID 1024

/* ---- reference block partition (src/stacking/stacking.c:1397-1476) and the libgomp
 *      schedule(static) assignment of blocks to OpenMP threads (:1513-1516) ---- */
struct Block {
	long channel, start_row, end_row;
};

static int make_blocks(long H, int nb_channels, int max_number_of_rows, int nb_threads,
		std::vector<Block> &blocks) {
	int size_of_stacks = max_number_of_rows / nb_threads;
	if (size_of_stacks == 0)
		size_of_stacks = 1;
	long nb_parallel_stacks;
	int remainder;
	if (H / size_of_stacks < 4) {
		nb_parallel_stacks = 4 * nb_channels;
		size_of_stacks = (int)(H / 4);
		remainder = (int)(H % 4);
	} else {
		nb_parallel_stacks = H * nb_channels / size_of_stacks;
		if (nb_parallel_stacks % nb_channels != 0 || (H * nb_channels) % size_of_stacks != 0) {
			nb_parallel_stacks += nb_channels - (nb_parallel_stacks % nb_channels);
			size_of_stacks = (int)(H * nb_channels / nb_parallel_stacks);
		}
		remainder = (int)(H - (nb_parallel_stacks / nb_channels * size_of_stacks));
	}
	if (size_of_stacks <= 0)
		return -1;
	blocks.clear();
	long channel = 0, row = 0, end;
	do {
		if ((long)blocks.size() >= nb_parallel_stacks)
			return -1;
		Block b;
		b.channel = channel;
		b.start_row = row;
		end = row + size_of_stacks - 1;
		if (remainder > 0) {
			end++;
			remainder--;
		}
		if (end >= H - 1 || (H - end < size_of_stacks / 10)) {
			end = H - 1;
			row = 0;
			channel++;
			remainder = (int)(H - (nb_parallel_stacks / nb_channels * size_of_stacks));
		} else {
			row = end + 1;
		}
		b.end_row = end;
		blocks.push_back(b);
	} while (channel < nb_channels);
	return (long)blocks.size() == nb_parallel_stacks ? 0 : -1;
}

static void omp_static_chunk(long n, int nthr, int t, long *begin, long *end) {
	long q = n / nthr, r = n % nthr;
	if (t < r) {
		q++;
		*begin = q * t;
	} else {
		*begin = q * t + r;
	}
	*end = *begin + q;
}

static int default_threads(void) {
	long n = sysconf(_SC_NPROCESSORS_ONLN);
	return n > 0 ? (int)n : 1;
}

static int pick_nreg(int N) {
	if (N <= 64) return 1;
	if (N <= 128) return 2;
	if (N <= 256) return 4;
	if (N <= 512) return 8;
	if (N <= 1024) return 16;
	return 0;
}

/* k_stack_literal: one thread per queued pixel with N * 5 bytes of scratch each; SG_LIT_THREADS
 * threads up to 2048 frames, then as many as 1 GiB of scratch holds (at least 4096) */
static unsigned lit_thread_count(int N) {
	const size_t lit_bytes = ((size_t)N * 5 + 15) & ~(size_t)15;
	return (unsigned)std::max<size_t>(4096, std::min<size_t>(SG_LIT_THREADS, ((size_t)1 << 30) / lit_bytes) & ~(size_t)63);
}
static size_t lit_scratch_bytes(int N) {
	return (size_t)lit_thread_count(N) * (((size_t)N * 5 + 15) & ~(size_t)15);
}

/* SUM and MEAN without rejection add up to N samples of 65535 per pixel: N 65535 fits the reduce
 * kernels' uint32_t sums up to N = 65537 (2^32 - 1 exactly).  The reference sums in unsigned long
 * and double with no cap (stacking.c:196-355, :1790-1794), so a longer stack takes 64-bit sums */
#define SG_SUM_U32_MAXN 65537
static bool sg_sum_wide(int method, int N) {
	return (method == SG_STACK_SUM || method == SG_STACK_MEAN) && N > SG_SUM_U32_MAXN;
}

/* the main kernel of a call */
enum SgMainPath {
	SG_MAIN_REDUCE = 0,	/* k_stack_reduce: SUM / MEAN / MAX / MIN, one pixel per lane */
	SG_MAIN_REDUCE2,	/* k_stack_reduce2: a pixel pair per lane */
	SG_MAIN_REDUCE3,	/* k_stack_reduce3<m, seg>: XCD-aware SGPR-offset loads */
	SG_MAIN_SORTED,		/* k_stack_sorted<nreg, false> over every tile */
	SG_MAIN_HIST,		/* k_stack_hist<rj, norm> */
	SG_MAIN_LINFIT,		/* k_stack_linfit<km, nw> */
	SG_MAIN_LITERAL_ALL,	/* k_list_all: every pixel to the literal kernel */
	SG_MAIN_REDUCE_WIDE	/* k_stack_reduce_wide: SUM / MEAN of more than SG_SUM_U32_MAXN frames, 64-bit sums */
};
/* where the redo list of the histogram / linfit kernels goes */
enum SgRedoRoute {
	SG_REDO_NONE = 0,
	SG_REDO_REPLAY_THEN_SORTED,	/* up to rp_maxn pixels to k_stack_replay, a longer list to the sorted kernel */
	SG_REDO_SORTED,			/* k_stack_sorted<nreg, true> */
	SG_REDO_TO_LITERAL		/* k_redo_to_literal: N > 1024, no sorted kernel */
};

struct SgStackPlan {
	char err[512];			/* the message of a failed plan (sg_last_error's text) */
	/* the descriptor's scalars the kernels take as they are */
	int N, W, H, C, method, rejection;
	double sig0, sig1;
	int row_begin, row_end, nrows;
	bool result_at_collect;		/* SG_STACK_RESULT_AT_COLLECT: an async call's tail on the tail stream */
	/* SgStackParams fields derived from the descriptor and the knobs */
	int normalize, use_shift, sy_min, sy_max, res_begin, res_end;
	int hist_maxsx, hist_norm_fold, ztab_k1, ztab_k2, dbg, prio, wins_cap;
	/* host tables, as the device reads them (stage_inputs copies them in this order):
	 * sh: c1[Npad] int, sx2[Npad] int16, shiftx[N], shifty[N];
	 * nm (normalised stacks): offset[N], mul[N], scale[N], {scale, offset | mul}[Npad] pairs, then
	 *   k_norm_fma_check's Npad candidate pairs, its staged verdict word (at 3 N + 4 Npad) and its
	 *   integer offsets;
	 * tables (rejection / median stacks): blk_of_row[C H], then channel, start, end and the first
	 *   block of the owning OpenMP thread, nblocks entries each;
	 * ztab: int[8] per border row (SgStackParams::ztab) */
	int Npad;
	std::vector<int> sh;
	std::vector<double> nm;
	std::vector<int> tables, ztab;
	std::vector<Block> blocks;
	int nblocks;
	unsigned int staged_verdict;
	/* the route */
	bool hist_addr_ok;		/* the shifted row offsets of a plane fit the 32-bit forms */
	bool rejection_family;		/* MEDIAN or MEAN with rejection: flag map, chain tables, literal phases */
	bool sum;			/* SUM: the raw sums and the maximum */
	bool wide;			/* SUM / MEAN without rejection past SG_SUM_U32_MAXN frames: 64-bit sums and maximum */
	int main;			/* SgMainPath */
	int nreg, rj, norm, km, nw, seg, m;
	bool linfit_tables;		/* k_linfit_tables runs first */
	bool norm_check;		/* k_norm_fma_check runs before the main kernel */
	bool compact;
	size_t cmp_cap;
	int redo;			/* SgRedoRoute */
	unsigned int list_minn, rp_maxn;	/* SG_REDO_REPLAY_MAX on the replay route, else 0 */
	int replay_nm;			/* k_stack_replay<replay_nm> runs (0: it does not) */
	/* launch shapes */
	unsigned int main_grid[3], main_threads;	/* main_threads 0: sgh_block_threads(rj) */
	size_t main_lds, sorted_lds;
	unsigned int fin_grid_x;	/* k_sum_finalize: (fin_grid_x, rows, C) */
	size_t npix_img, npix_launch;
	unsigned int lit_threads;
	size_t scratch_bytes;
	/* sg_stack_stats as the launch step leaves them (k_sum_finalize adds its launch) */
	int path, launches, main_kernel_blocks, norm_fma;
	int hist_ldspad;		/* occupancy report of a probe build */
};

static int sg_plan_fail(SgStackPlan &pl, int code, const char *fmt, ...) {
	va_list ap;
	va_start(ap, fmt);
	vsnprintf(pl.err, sizeof pl.err, fmt, ap);
	va_end(ap);
	return code;
}

/* the checks in front of everything else: a call they refuse leaves the statistics alone */
static int sg_stack_plan_args(const sg_stack_desc *d, int row_begin, int row_end, SgStackPlan &pl) {
	pl.err[0] = 0;
	if (d->nb_frames < 2)
		return sg_plan_fail(pl, SG_ERR_GENERIC, "select at least two frames (%ld)", (long)d->nb_frames);
	if (d->width <= 0 || d->height <= 0 || d->nb_layers < 1 || d->nb_layers > 3 || row_begin < 0 ||
			row_end > d->height || row_begin >= row_end)
		return sg_plan_fail(pl, SG_ERR_SIZE, "bad geometry 0");
	if (d->method < 0 || d->method > 4)
		return sg_plan_fail(pl, SG_ERR_GENERIC, "unknown method %ld", (long)d->method);
	return SG_OK;
}

/* range of the row shifts the stack applies (0, 0 without shifts; stack_median ignores them) */
static bool sg_plan_shift_range(const sg_stack_desc *d, int *sy_min, int *sy_max) {
	const bool use_shift = d->method != SG_STACK_MEDIAN && d->shiftx && d->shifty;
	*sy_min = *sy_max = 0;
	for (int i = 0; use_shift && i < d->nb_frames; i++) {
		*sy_min = i ? std::min(*sy_min, d->shifty[i]) : d->shifty[i];
		*sy_max = i ? std::max(*sy_max, d->shifty[i]) : d->shifty[i];
	}
	return use_shift;
}

/* the resident rows and the frame rows the band's output rows read (R - shifty, :1550-1577) */
static int sg_plan_residency(const sg_stack_desc *d, SgStackPlan &pl) {
	pl.res_begin = 0;
	pl.res_end = pl.H;
	if (d->resident_rows[0] != 0 || d->resident_rows[1] != 0) {
		pl.res_begin = d->resident_rows[0];
		pl.res_end = d->resident_rows[1];
		if (pl.res_begin < 0 || pl.res_end > pl.H || pl.res_begin >= pl.res_end)
			return sg_plan_fail(pl, SG_ERR_SIZE, "bad resident row range %ld", (long)pl.res_begin);
	}
	const int lo = (int)std::max<int64_t>(0, (int64_t)pl.row_begin - pl.sy_max);
	const int hi = (int)std::min<int64_t>(pl.H - 1, (int64_t)pl.row_end - 1 - pl.sy_min);
	if (lo <= hi && (lo < pl.res_begin || hi >= pl.res_end))
		return sg_plan_fail(pl, SG_ERR_SIZE, "frame rows %d..%d read by the band are not all resident (%d..%d)", lo, hi,
				pl.res_begin, pl.res_end - 1);
	return SG_OK;
}

/* per frame c1 = shifty*W*2 + 2*shiftx and sx2 = 2*shiftx for the histogram path (zeros when
 * there is no registration data), then the plain shift arrays */
static void sg_plan_shift_table(const sg_stack_desc *d, SgStackPlan &pl) {
	const int N = pl.N, Npad = pl.Npad, W = pl.W, H = pl.H;
	pl.sh.assign((size_t)Npad + Npad / 2 + 2 * N, 0);
	/* the histogram path addresses a frame plane with 32-bit offsets: (R - sy) W 2 must fit */
	pl.hist_addr_ok = (int64_t)H * W * 2 <= (1ll << 30);
	pl.hist_maxsx = 0;
	if (!pl.use_shift)
		return;
	int16_t *sx2 = (int16_t *)(pl.sh.data() + Npad);
	for (int i = 0; i < N; i++) {
		const int64_t sy = d->shifty[i], sx = d->shiftx[i];
		const int64_t asy = sy < 0 ? -sy : sy, asx = sx < 0 ? -sx : sx;
		if ((int64_t)(H + asy) * W * 2 + 2 * asx >= (1ll << 31) || asx > 16383)
			pl.hist_addr_ok = false;
		pl.sh[i] = (int)(sy * W * 2 + 2 * sx);
		sx2[i] = (int16_t)(2 * sx);
		if (asx > pl.hist_maxsx)
			pl.hist_maxsx = (int)asx;
	}
	memcpy(pl.sh.data() + Npad + Npad / 2, d->shiftx, sizeof(int) * N);
	memcpy(pl.sh.data() + Npad + Npad / 2 + N, d->shifty, sizeof(int) * N);
}

/* normalisation coefficients, the histogram path's pairs and the additive fold decision */
static void sg_plan_norm_table(const sg_stack_desc *d, const SgKnobs &k, SgStackPlan &pl) {
	const int N = pl.N, Npad = pl.Npad;
	pl.hist_norm_fold = 0;
	/* the word k_norm_fma_check starts from (bit 0: no fma load, bit 1: no integer load; the check
	 * ORs in what it finds) and the histogram kernel reads as the load verdict.  This is the one
	 * place it is computed: SG_NORM_FMA 0 -> 3 (neither form; the check does not run), 1 -> 2 (the
	 * fma only), 2 (default) -> 0 (the integer form first) */
	pl.staged_verdict = k.norm_fma == 0 ? 3u : (k.norm_fma == 1 ? 2u : 0u);
	if (!pl.normalize)
		return;
	std::vector<double> &nm = pl.nm;
	/* + the pairs, Npad single-rounding candidate pairs, the verdict word and the integer offsets
	 * of k_norm_fma_check's scale-1 form */
	nm.assign((size_t)3 * N + 6 * Npad + 2, 0.0);
	for (int i = 0; i < N; i++) {
		nm[i] = d->offset ? d->offset[i] : 0.0;
		nm[N + i] = d->mul ? d->mul[i] : 1.0;
		nm[2 * N + i] = d->scale ? d->scale[i] : 1.0;
	}
	memcpy(&nm[3 * N + 4 * Npad], &pl.staged_verdict, sizeof pl.staged_verdict);
	/* the histogram path's per-frame pair {scale, offset} (additive) or {scale, mul}
	 * (multiplicative), read with one scalar load per frame */
	const bool additive = pl.normalize == SG_ADDITIVE || pl.normalize == SG_ADDITIVE_SCALING;
	/* additive: when every offset - 0.5 is exact (TwoSum error 0), the pair carries
	 * offset - 0.5 and the kernel folds round_to_WORD's + 0.5 into the subtraction
	 * (NORM 3: trunc(v scale - (offset - 0.5)), one fp64 add per sample less; equal to
	 * trunc((v scale - offset) + 0.5) whenever the fold is exact, tests/test_norm_fold.py) */
	bool fold = additive;
	for (int i = 0; fold && i < N; i++) {
		const double b = nm[i], c = b - 0.5, bb = c - b;
		fold = ((b - (c - bb)) + (-0.5 - bb)) == 0.0;
	}
	pl.hist_norm_fold = fold ? 1 : 0;
	for (int i = 0; i < N; i++) {
		nm[3 * N + 2 * i] = nm[2 * N + i];
		nm[3 * N + 2 * i + 1] = additive ? (fold ? nm[i] - 0.5 : nm[i]) : nm[N + i];
	}
}

/* additive normalisation with shifts: a row whose shifted source row leaves frame f holds
 * f's normalised zero round_to_WORD(0 scale - offset) (:1550-1577 zero fill, then
 * :1635-1652); the histogram path takes those values per border row from this table
 * (SghPix::zmax) instead of sending the rows to the redo list */
static void sg_plan_ztab(const sg_stack_desc *d, SgStackPlan &pl) {
	const int N = pl.N, H = pl.H;
	pl.ztab_k1 = pl.ztab_k2 = 0;
	if (!(pl.use_shift && (pl.normalize == SG_ADDITIVE || pl.normalize == SG_ADDITIVE_SCALING)))
		return;
	int k1 = std::max(0, pl.sy_max), k2 = std::max(0, -pl.sy_min);
	if (k1 + k2 >= H) {
		k1 = H;
		k2 = 0;
	}
	pl.ztab.assign((size_t)8 * (k1 + k2), 0);
	bool any = false;
	for (int t = 0; t < k1 + k2; t++) {
		const int R = t < k1 ? t : H - k2 + (t - k1);
		int zc = 0, zmin = 65535, zmax = 0;
		long long zs = 0, zss = 0;	/* 64-bit: N up to 65535 normalised zeros up to 65534 */
		for (int f = 0; f < N; f++) {
			const int sr = R - d->shifty[f];
			if (sr >= 0 && sr < H)
				continue;
			const double x = 0.0 * pl.nm[2 * N + f] - pl.nm[f];	/* v scale - offset at v = 0 */
			const int z = x <= 0.0 ? 0 : (x > 65535.0 ? 65535 : (int)(x + 0.5));
			if (z == 0 || z == 65535)
				continue;
			zc++;
			zs += z;
			zss += (long long)z * z;
			zmin = std::min(zmin, z);
			zmax = std::max(zmax, z);
		}
		if (!zc)
			continue;
		any = true;
		int *e = &pl.ztab[(size_t)8 * t];
		e[0] = zc;
		e[1] = (int)(uint32_t)(zs & 0xFFFFFFFFll);
		e[6] = (int)(zs >> 32);
		e[2] = (int)(uint32_t)(zss & 0xFFFFFFFFll);
		e[3] = (int)(zss >> 32);
		e[4] = zmin;
		e[5] = zmax;
	}
	if (any) {
		pl.ztab_k1 = k1;
		pl.ztab_k2 = k2;
	} else {
		pl.ztab.clear();
	}
}

/* stack_mean_with_rejection reads a block's rows with area.y += shifty; when a block that
 * does not start at the top (area.y > 0) is shifted partly above the frame (area.y + shifty
 * < 0 <= area.y + h - 1 + shifty) it places the rows it reads at offset W (area.y - shifty)
 * instead of W (-area.y - shifty) (src/stacking/stacking.c:1555-1561): the rows land 2 area.y
 * too low and run 2 area.y + h - largest_block_h rows past its block buffer, always a heap
 * overflow (the neighbouring buffer or the allocator's data).  No defined result exists to
 * reproduce, so the call refuses the shifts instead of zero filling silently */
static int sg_plan_block_overflow(const sg_stack_desc *d, SgStackPlan &pl) {
	for (const Block &b : pl.blocks) {
		const long ay = b.start_row, ah = b.end_row - b.start_row + 1;
		if (!(ay > 0 && ay + pl.sy_min < 0 && ay + ah - 1 + pl.sy_max >= 0))
			continue;
		bool hit = false;
		for (int i = 0; i < pl.N && !hit; i++)
			hit = ay + d->shifty[i] < 0 && ay + ah - 1 + d->shifty[i] >= 0;
		if (hit)
			return sg_plan_fail(pl, SG_ERR_GENERIC, "a registration shift of %d rows reaches above the block starting at "
					"row %ld: the reference overflows its block buffer there (stacking.c:1555-1561); "
					"use more rows per block (max_number_of_rows / fewer threads)", pl.sy_min, ay);
	}
	return SG_OK;
}

/* the reference's block partition, once per call: the overflow refusal above, then (rejection /
 * median stacks) the thread order tables of the stale-state chains */
static int sg_plan_blocks(const sg_stack_desc *d, SgStackPlan &pl) {
	const int H = pl.H, C = pl.C;
	const bool overflow_check = pl.method == SG_STACK_MEAN && pl.use_shift && pl.sy_min < 0;
	pl.nblocks = 0;
	if (!overflow_check && !pl.rejection_family)
		return SG_OK;
	const int nthr = d->max_thread > 0 ? d->max_thread : default_threads();
	const int maxrows = d->max_number_of_rows > 0 ? d->max_number_of_rows : H;
	const int part = make_blocks(H, C, maxrows, nthr, pl.blocks);
	if (overflow_check && part == 0)
		if (int rc = sg_plan_block_overflow(d, pl))
			return rc;
	if (!pl.rejection_family)	/* a plain MEAN ignores a partition that fails */
		return SG_OK;
	if (part)
		return sg_plan_fail(pl, SG_ERR_GENERIC, "block partition failed (the reference would read "
				"uninitialised blocks)0");
	const int nb = (int)pl.blocks.size();
	pl.tables.assign((size_t)C * H + 4 * nb, 0);
	int *blk_of_row = pl.tables.data(), *bch = blk_of_row + (size_t)C * H, *bst = bch + nb, *ben = bst + nb,
	    *bfi = ben + nb;
	for (int b = 0; b < nb; b++) {
		bch[b] = (int)pl.blocks[b].channel;
		bst[b] = (int)pl.blocks[b].start_row;
		ben[b] = (int)pl.blocks[b].end_row;
		for (long r = pl.blocks[b].start_row; r <= pl.blocks[b].end_row; r++)
			blk_of_row[(size_t)pl.blocks[b].channel * H + r] = b;
	}
	for (int t = 0; t < nthr; t++) {
		long b0, b1;
		omp_static_chunk(nb, nthr, t, &b0, &b1);
		for (long b = b0; b < b1; b++)
			bfi[b] = (int)b0;
	}
	pl.nblocks = nb;
	return SG_OK;
}

/* the histogram main kernel's template arguments, its compact side list and the
 * load check */
static void sg_plan_hist(const SgKnobs &k, SgStackPlan &pl) {
	const int N = pl.N, W = pl.W, C = pl.C, nrows = pl.nrows;
	/* REJ: 2 SIGMA, 4 WINSORIZED, 1 PERCENTILE, 3 SIGMEDIAN, 8 stack_median */
	pl.rj = pl.method == SG_STACK_MEDIAN ? 8 : pl.rejection == SG_WINSORIZED ? 4 :
		pl.rejection == SG_PERCENTILE ? 1 : pl.rejection == SG_SIGMEDIAN ? 3 : 2;
	/* a tile = 128 pixels of a row (sg_stack_hist.hip) */
	pl.main_grid[0] = (unsigned)((size_t)((W + 127) / 128) * nrows * C);
	pl.main_threads = 0;
	pl.main_lds = (size_t)k.hist_ldspad;
	/* normalised SIGMA / WINSORIZED: redo pixels whose samples the tile fully knows leave
	 * their sorted columns for the sorted kernel (sgh_compact), up to a 384 MiB buffer */
	pl.compact = pl.norm != 0 && (pl.rj == 2 || pl.rj == 4) && pl.nreg && k.hist_compact;
	if (pl.compact)
		pl.cmp_cap = std::min<size_t>(pl.npix_launch, k.hist_compact >= 2 ?
				(size_t)k.hist_compact : ((size_t)384 << 20) / ((size_t)N * 2));
	/* normalised: check the single-rounding load against the reference's operations over every
	 * u16 value of every frame (k_norm_fma_check, ~10 us); the kernel reads the verdict.
	 * norm_fma: the best load allowed; the verdict replaces it when the call is folded */
	pl.norm_check = pl.norm != 0 && k.norm_fma;
	if (pl.norm_check)
		pl.norm_fma = pl.norm != 2 && k.norm_fma == 2 ? 2 : 1;
}

/* LINEARFIT's decision-exact kernel: one workgroup per 64 pixels of a row, the tile's columns
 * in LDS */
static void sg_plan_linfit(const SgKnobs &k, SgStackPlan &pl) {
	pl.km = pl.N <= 512 ? 8 : 16;
	/* waves per tile: 4, 8 or (KM = 8 only: 187 VGPRs at KM = 16) 16 */
	pl.nw = k.linfit_waves == 4 ? 4 : (k.linfit_waves == 16 && pl.km == 8) ? 16 : 8;
	pl.main_grid[0] = (unsigned)((size_t)((pl.W + 63) / 64) * pl.nrows * pl.C);
	pl.main_threads = 64u * pl.nw;
	pl.main_lds = (size_t)64 * (64 * pl.km + 2) * sizeof(uint16_t);
}

/* MEDIAN and MEAN with rejection: histogram / linfit / sorted / literal-all, the redo route of
 * the first two, the replay and literal kernels behind all of them */
static void sg_plan_rejection_route(const sg_stack_desc *d, const SgKnobs &k, SgStackPlan &pl) {
	const int N = pl.N, W = pl.W, C = pl.C, nrows = pl.nrows;
	const bool mean = pl.method == SG_STACK_MEAN, median = pl.method == SG_STACK_MEDIAN;
	const bool sigma_wins = mean && (pl.rejection == SG_SIGMA || pl.rejection == SG_WINSORIZED);
	pl.nreg = pick_nreg(N);
	/* LINEARFIT's decision-exact kernel (k_stack_linfit, sg_stack.hip) takes the histogram
	 * path's place: its redo list goes to the sorted kernel's exact replay the same way */
	const bool linfit_fast = d->kernel_path != SG_PATH_SORTED && mean && pl.rejection == SG_LINEARFIT && N >= 16 &&
		N <= 1024 && k.linfit_fast;
	/* histogram fast path (sg_stack_hist.hip): SIGMA / WINSORIZED / PERCENTILE / SIGMEDIAN rejection
	 * and stack_median, any normalisation, 16 <= N <= 65535 (per-lane zero / 65535 counters are
	 * 16-bit halves) */
	const bool hist = !linfit_fast && d->kernel_path != SG_PATH_SORTED && N >= 16 && N <= 65535 && pl.hist_addr_ok &&
		(median || (mean && (pl.rejection == SG_SIGMA || pl.rejection == SG_WINSORIZED ||
				pl.rejection == SG_PERCENTILE || (pl.rejection == SG_SIGMEDIAN && k.hist_sigmedian))));
	/* beyond the sorted kernel's 1024 frames a stack without a histogram path (LINEARFIT, or
	 * planes past the histogram's 32-bit offsets) goes to the literal kernel pixel by pixel: slow,
	 * but any N as the reference (:1486-1507) */
	pl.main = linfit_fast ? SG_MAIN_LINFIT : hist ? SG_MAIN_HIST : pl.nreg ? SG_MAIN_SORTED : SG_MAIN_LITERAL_ALL;
	pl.npix_launch = (size_t)C * nrows * W;
	pl.linfit_tables = mean && pl.rejection == SG_LINEARFIT;
	const size_t nblk = (size_t)((W + SG_TILE_W - 1) / SG_TILE_W) * nrows * C;
	/* LINEARFIT: + one rejected[] bit per frame and pixel of the tile (reject_linearfit) */
	pl.sorted_lds = (size_t)N * SG_STAGE_STRIDE * 2 + (pl.rejection == SG_LINEARFIT ? (size_t)64 * ((N + 31) / 32) * 4 : 0);
	/* NORM: 0 none, 1 additive (round(v scale - offset)), 2 multiplicative (round(v scale mul)),
	 * 3 additive with the folded + 0.5 */
	pl.norm = pl.normalize == SG_NO_NORM ? 0 :
		(pl.normalize == SG_ADDITIVE || pl.normalize == SG_ADDITIVE_SCALING) ? (pl.hist_norm_fold ? 3 : 1) : 2;
	pl.launches = 1;
	if (pl.main == SG_MAIN_HIST)
		sg_plan_hist(k, pl);
	else if (pl.main == SG_MAIN_LINFIT)
		sg_plan_linfit(k, pl);
	else if (pl.main == SG_MAIN_SORTED) {
		pl.main_grid[0] = (unsigned)nblk;
		pl.main_threads = SG_SORT_THREADS;
		pl.main_lds = pl.sorted_lds;
	} else {
		pl.main_grid[0] = 1024;
		pl.main_threads = 256;
	}
	if (pl.main != SG_MAIN_LITERAL_ALL)
		pl.main_kernel_blocks = (int)nblk;
	if (pl.main == SG_MAIN_HIST || pl.main == SG_MAIN_LINFIT) {
		pl.path = 1;
		/* the redo pixels, routed on the device (no host round trip in the call):
		 * - SIGMA / WINSORIZED, N <= SG_REPLAY_MAXN: up to SG_REDO_REPLAY_MAX pixels straight to
		 *   the wave-per-pixel replay (every sample of a pixel gathered by one wave at once), a
		 *   longer list (rare: e.g. normalised zeros of rows near the frame border) through the
		 *   sorted kernel (measured: 22 k pixels faster in the replay, 113 k slower);
		 * - stack_median / PERCENTILE: the sorted kernel (the literal kernel's one thread per
		 *   pixel sorts slowly: 740 pixels took 8 ms);
		 * - N > 1024 (no sorted kernel): every redo pixel to the replay / literal kernels */
		pl.redo = (pl.nreg && sigma_wins && N <= SG_REPLAY_MAXN && k.redo_replay) ? SG_REDO_REPLAY_THEN_SORTED :
			pl.nreg ? SG_REDO_SORTED : SG_REDO_TO_LITERAL;
		if (pl.redo == SG_REDO_REPLAY_THEN_SORTED)
			pl.list_minn = pl.rp_maxn = SG_REDO_REPLAY_MAX;	/* the sorted kernel idles unless the list is longer */
		pl.launches += (pl.compact ? 1 : 0) + 1;
	}
	/* exact wave-per-pixel replay of queued SIGMA / WINSORIZED pixels (the replay route's redo
	 * list, early breaks with this pixel's own stale rejected[]), then the literal path for what
	 * remains: two phases, grids read the count on the device.  The per-wave LDS of
	 * k_stack_replay<512> is sized for 512 frames (SG_REPLAY_FASTN) */
	pl.replay_nm = (sigma_wins && N <= SG_REPLAY_MAXN) ? (N <= 512 ? 512 : SG_REPLAY_MAXN) : 0;
	pl.lit_threads = lit_thread_count(N);
	pl.scratch_bytes = lit_scratch_bytes(N);
	pl.launches += (pl.replay_nm ? 1 : 0) + 2;
}

/* SUM / MEAN without rejection / MAX / MIN */
static void sg_plan_reduce_route(const SgKnobs &k, SgStackPlan &pl) {
	const int W = pl.W, H = pl.H, C = pl.C, nrows = pl.nrows;
	/* pixel pairs per lane (dword loads) unless a plane is too large for a 31-bit offset */
	const bool pairs = W >= 2 && (uint64_t)W * (uint64_t)H * 2u < (1ull << 31) && k.reduce1 != 1;
	/* XCD-aware SGPR-offset loads (k_stack_reduce3) when the shifted row offsets fit 32 bits,
	 * the per-lane pair kernel (SG_REDUCE1=2, A/B) otherwise */
	const bool r3 = pairs && pl.hist_addr_ok && k.reduce1 == 0;
	/* 256-byte segments per wave: SEG = 1 by default (SG_REDUCE_SEG: 1 / 2 / 4, A/B; 2 and 4
	 * measured slower, profiles/r05g_reduce_seg_*) */
	pl.seg = k.reduce_seg;
	/* MEAN: the normalising instance's fp64 path costs registers: its own kernel */
	pl.m = pl.method == SG_STACK_SUM ? 0 : pl.method == SG_STACK_MEAN ? (pl.normalize ? 2 : 1) :
		pl.method == SG_STACK_MAX ? 3 : 4;
	/* more frames than uint32_t sums hold: the one-pixel-per-lane kernel with 64-bit sums (any
	 * plane size; MAX and MIN never overflow and keep their route) */
	pl.wide = sg_sum_wide(pl.method, pl.N);
	pl.main = pl.wide ? SG_MAIN_REDUCE_WIDE : r3 ? SG_MAIN_REDUCE3 : pairs ? SG_MAIN_REDUCE2 : SG_MAIN_REDUCE;
	pl.fin_grid_x = (unsigned)((W + 255) / 256);
	pl.main_threads = 256;
	pl.main_grid[1] = (unsigned)nrows;
	pl.main_grid[2] = (unsigned)C;
	if (pl.wide) {
		pl.main_grid[0] = pl.fin_grid_x;
	} else if (r3) {
		pl.main_grid[0] = (unsigned)(((W + 512 * pl.seg - 1) / (512 * pl.seg)) * (size_t)nrows * C);
		pl.main_grid[1] = pl.main_grid[2] = 1;
	} else {
		pl.main_grid[0] = pairs ? (unsigned)(((W + 1) / 2 + 255) / 256) : pl.fin_grid_x;
	}
	pl.main_kernel_blocks = (int)(pl.main_grid[0] * pl.main_grid[1] * pl.main_grid[2]);
	pl.launches = 1;
}

/*
 * plan the stack of rows [row_begin, row_end) of *d under the knobs k.  SG_OK, or the call's
 * return code with its message in pl.err; a failed plan is not launched.
 */
static int sg_stack_plan(const sg_stack_desc *d, int row_begin, int row_end, const SgKnobs &k, SgStackPlan &pl) {
	pl = SgStackPlan();	/* every field zero, the tables empty */
	if (int rc = sg_stack_plan_args(d, row_begin, row_end, pl))
		return rc;
	pl.N = d->nb_frames;
	pl.W = d->width;
	pl.H = d->height;
	pl.C = d->nb_layers;
	pl.method = d->method;
	pl.rejection = d->rejection;
	pl.sig0 = d->sig[0];
	pl.sig1 = d->sig[1];
	pl.row_begin = row_begin;
	pl.row_end = row_end;
	pl.nrows = row_end - row_begin;
	pl.result_at_collect = (d->flags & SG_STACK_RESULT_AT_COLLECT) != 0;
	pl.normalize = (d->method == SG_STACK_MEAN || d->method == SG_STACK_MEDIAN) ? d->normalize : 0;
	pl.use_shift = sg_plan_shift_range(d, &pl.sy_min, &pl.sy_max);
	pl.dbg = k.hist_dbg;
	pl.prio = k.hist_prio;	/* 1 measured best: 4.73 -> 4.58 ms (scripts/gpu_prio.sh) */
	pl.wins_cap = k.wins_cap;
	pl.hist_ldspad = k.hist_ldspad;
	pl.Npad = (pl.N + 15) & ~15;	/* histogram-path table: 64-byte aligned, padded */
	pl.npix_img = (size_t)pl.C * pl.H * pl.W;
	pl.rejection_family = d->method == SG_STACK_MEDIAN || (d->method == SG_STACK_MEAN && d->rejection != SG_NO_REJEC);
	pl.sum = d->method == SG_STACK_SUM;
	pl.main_grid[0] = pl.main_grid[1] = pl.main_grid[2] = 1;
	if (int rc = sg_plan_residency(d, pl))
		return rc;
	sg_plan_shift_table(d, pl);
	sg_plan_norm_table(d, k, pl);
	sg_plan_ztab(d, pl);
	if (int rc = sg_plan_blocks(d, pl))
		return rc;
	if (pl.rejection_family)
		sg_plan_rejection_route(d, k, pl);
	else
		sg_plan_reduce_route(k, pl);
	return SG_OK;
}

/* the plan's share of the kernels' parameter block (the launch step adds the device pointers) */
static void sg_plan_params(const SgStackPlan &pl, SgStackParams &p) {
	memset(&p, 0, sizeof p);
	p.N = pl.N;
	p.W = pl.W;
	p.H = pl.H;
	p.C = pl.C;
	p.method = pl.method;
	p.rejection = pl.rejection;
	p.normalize = pl.normalize;
	p.sig0 = pl.sig0;
	p.sig1 = pl.sig1;
	p.use_shift = pl.use_shift;
	p.row_begin = pl.row_begin;
	p.row_end = pl.row_end;
	p.res_begin = pl.res_begin;
	p.res_end = pl.res_end;
	p.sy_min = pl.sy_min;
	p.sy_max = pl.sy_max;
	p.dbg = pl.dbg;
	p.prio = pl.prio;
	p.wins_cap = pl.wins_cap;
	p.hist_npad = pl.Npad;
	p.hist_maxsx = pl.hist_maxsx;
	p.hist_norm_fold = pl.hist_norm_fold;
	p.ztab_k1 = pl.ztab_k1;
	p.ztab_k2 = pl.ztab_k2;
}
