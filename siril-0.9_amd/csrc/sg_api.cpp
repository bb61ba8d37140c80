/*
 * sg_api.cpp - C ABI of libsirilgpu.so (include/sirilgpu.h): contexts, HBM workspaces,
 * kernel selection and the host-pull stacking path.
 *
 * Everything here is plumbing around the gfx950 kernels of sg_stack.hip / sg_register.hip;
 * no pixel is ever computed on the host.  If a launch fails the call fails loudly
 * (SG_ERR_DEVICE + sg_last_error), there is no CPU fallback.
 */
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <unistd.h>
#include <vector>
#include <string>
#include <algorithm>
#include <array>
#include <atomic>
#include <mutex>
#include <thread>
#include "sg_common.hpp"
#include "../../include/sirilgpu.h"

struct SgChainTables {
	const int *blk_of_row;
	const int *blk_channel, *blk_start, *blk_end, *blk_first;
	int nblocks;
};

template <int NREG, bool LISTED>
__global__ void k_stack_sorted(SgStackParams p, const unsigned int *list, const unsigned int *list_count);
template <int REJ, int NORM>
__global__ void k_stack_hist(SgStackParams p, const int *tab, const int4 *norm, unsigned int *redo_count,
		unsigned int *redo_list);
__global__ void k_norm_fma_check(double *pairs, int N, int npad, int mode, unsigned int *verdict);
template <int KM, int NW>
__global__ void k_stack_linfit(SgStackParams p, unsigned int *redo_count, unsigned int *redo_list);
void sg_dbg_why_dump(hipStream_t s);
int sgh_block_threads(int rej);
template <int NM>
__global__ void k_stack_replay(SgStackParams p);
__global__ void k_redo_to_literal(SgStackParams p, const unsigned int *list, const unsigned int *count,
		unsigned int maxn);
__global__ void k_stack_reduce(SgStackParams p);
__global__ void k_stack_reduce2(SgStackParams p);
template <int M, int SEG>
__global__ void k_stack_reduce3(SgStackParams p, const int *tab, const int *shifty);
__global__ void k_sum_finalize(SgStackParams p);
__global__ void k_stack_reduce_wide(SgStackParams p);
__global__ void k_sum_finalize_wide(SgStackParams p);
__global__ void k_stack_literal(SgStackParams p, SgChainTables t, unsigned int count, uint8_t *scratch, int phase);
__global__ void k_synth_fill(uint16_t *frames, int first_frame, int nframes, int C, int H, int W, int row_begin,
		int row_end, uint64_t seed, int maxshift, int64_t frame_stride, int64_t plane_stride);

#include "sg_ctx.hpp"
#include "sg_stack_plan.hpp"

__global__ void k_flip_rows(const uint16_t *src, uint16_t *dst, int W, int rows);
__global__ void k_stage_copy(uint4 *dst, const uint4 *src, unsigned int n16);
__global__ void k_linfit_tables(double *tab, int nmax);
__global__ void k_list_all(SgStackParams p);
__global__ void k_ctr_finalize(unsigned long long *ctr, unsigned long long *host);
/* host-pull readers per device and the bytes of one region read (two pinned + two device
 * staging buffers of this size per reader) */
#define SG_PULL_READERS 8
#define SG_PULL_CHUNK_BYTES ((size_t)4 << 20)
/* rejection counter shards at the start of the counter block (SgDevice::ctr) */
static const size_t SG_CTR_REJB = sizeof(unsigned long long) * SG_REJ_SHARDS * 6;

extern "C" int sg_init(sg_ctx **out, int ndev, const int *devs) {
	if (!out)
		return SG_ERR_GENERIC;
	*out = nullptr;
	int count = 0;
	if (hipGetDeviceCount(&count) != hipSuccess || count <= 0)
		return SG_ERR_DEVICE;
	sg_ctx *ctx = new sg_ctx();
	memset(&ctx->stats, 0, sizeof ctx->stats);
	ctx->knobs.read();
	if (ndev < 0) {	/* every visible device */
		ndev = count;
		devs = nullptr;
	}
	if (ndev == 0)
		ndev = 1;
	for (int i = 0; i < ndev; i++) {
		SgDevice d;
		d.id = devs ? devs[i] : i;
		if (d.id < 0 || d.id >= count) {
			delete ctx;
			return SG_ERR_DEVICE;
		}
		if (hipSetDevice(d.id) != hipSuccess || hipStreamCreateWithFlags(&d.stream, hipStreamNonBlocking) != hipSuccess) {
			delete ctx;
			return SG_ERR_DEVICE;
		}
		for (int k = 0; k < 4; k++)
			(void)hipEventCreate(&d.ev[k]);
		for (int k = 0; k < 2; k++) {
			for (int j = 0; j < 3; j++)
				(void)hipEventCreate(&d.cev[k][j]);
			(void)hipEventCreateWithFlags(&d.sl[k].stage_ev, hipEventDisableTiming);
		}
		for (int k = 0; k < 2; k++)
			(void)hipEventCreateWithFlags(&d.io_ev[k], hipEventDisableTiming);
		ctx->dev.push_back(d);
	}
	for (auto &a : ctx->dev)
		for (auto &b : ctx->dev)
			a.shared += (&a != &b && a.id == b.id) ? 1 : 0;
	*out = ctx;
	return SG_OK;
}

extern "C" void sg_shutdown(sg_ctx *ctx) {
	if (!ctx)
		return;
	for (auto &d : ctx->dev) {
		(void)hipSetDevice(d.id);
		(void)hipStreamSynchronize(d.stream);
		if (d.tail)
			(void)hipStreamSynchronize(d.tail);
		SgBuf *bufs[] = {&d.sum_buf, &d.frames, &d.out, &d.reg_sel, &d.reg_spec, &d.reg_work, &d.reg_tw, &d.reg_tw32,
			&d.reg_best, &d.reg_qbuf, &d.reg_qacc, &d.zeros, &d.io_raw, &d.io_bad, &d.warp_tab, &d.stats_buf, &d.ctr, &d.fs_work, &d.fs_plane, &d.fs_out,
			&d.fs_fit, &d.ecc_work, &d.cosme_work, &d.quality_work, &d.host_frames, &d.warp_work, &d.seqpsf_work, &d.starmatch_work};
		for (SgBuf *b : bufs)
			if (b->p)
				(void)hipFree(b->p);
		for (SgSlot &q : d.sl) {
			SgBuf *sb[] = {&q.inb, &q.flag_list, &q.flag_map, &q.redo, &q.cmp_cols, &q.cmp_list, &q.scratch, &q.lin_tab};
			for (SgBuf *b : sb)
				if (b->p)
					(void)hipFree(b->p);
			if (q.stage_h)
				(void)hipHostFree(q.stage_h);
			if (q.stage_ev)
				(void)hipEventDestroy(q.stage_ev);
		}
		if (d.tail)
			(void)hipStreamDestroy(d.tail);
		if (d.tail_ev)
			(void)hipEventDestroy(d.tail_ev);
		if (d.tail_done_ev)
			(void)hipEventDestroy(d.tail_done_ev);
		for (int k = 0; k < 2; k++)
			if (d.pinned[k])
				(void)hipHostFree(d.pinned[k]);
		if (d.ctr_h)
			(void)hipHostFree(d.ctr_h);
		for (int k = 0; k < 2; k++) {
			if (d.io_stage[k])
				(void)hipHostFree(d.io_stage[k]);
			if (d.io_ev[k])
				(void)hipEventDestroy(d.io_ev[k]);
		}
		for (int k = 0; k < 4; k++)
			if (d.ev[k])
				(void)hipEventDestroy(d.ev[k]);
		for (int k = 0; k < 2; k++)
			if (d.warp_ev[k])
				(void)hipEventDestroy(d.warp_ev[k]);
		for (int k = 0; k < 2; k++)
			for (int j = 0; j < 3; j++)
				if (d.cev[k][j])
					(void)hipEventDestroy(d.cev[k][j]);
		for (SgReader &rd : d.readers) {
			if (rd.stream)
				(void)hipStreamSynchronize(rd.stream);
			for (int k = 0; k < 2; k++) {
				if (rd.pin[k])
					(void)hipHostFree(rd.pin[k]);
				if (rd.dstage[k])
					(void)hipFree(rd.dstage[k]);
				if (rd.ev[k])
					(void)hipEventDestroy(rd.ev[k]);
			}
			if (rd.stream)
				(void)hipStreamDestroy(rd.stream);
		}
		if (d.aux) {
			(void)hipStreamSynchronize(d.aux);
			(void)hipStreamDestroy(d.aux);
		}
		for (int k = 0; k < 2; k++)
			if (d.aux_ev[k])
				(void)hipEventDestroy(d.aux_ev[k]);
		if (d.qacc_h)
			(void)hipHostFree(d.qacc_h);
		if (d.aux2) {
			(void)hipStreamSynchronize(d.aux2);
			(void)hipStreamDestroy(d.aux2);
		}
		for (int k = 0; k < 2; k++)
			if (d.aux2_ev[k])
				(void)hipEventDestroy(d.aux2_ev[k]);
		if (d.reg_pin)
			(void)hipHostFree(d.reg_pin);
		(void)hipStreamDestroy(d.stream);
	}
	delete ctx;
}

extern "C" const char *sg_last_error(const sg_ctx *ctx) {
	return ctx ? ctx->err.c_str() : "no context";
}

extern "C" int sg_get_last_stats(const sg_ctx *ctx, sg_stack_stats *st) {
	if (!ctx || !st)
		return SG_ERR_GENERIC;
	std::lock_guard<std::mutex> lk(((sg_ctx *)ctx)->mu);
	*st = ctx->stats;
	return SG_OK;
}

extern "C" int sg_device_count(const sg_ctx *ctx, int *ndev) {
	if (!ctx || !ndev)
		return SG_ERR_GENERIC;
	*ndev = (int)ctx->dev.size();
	return SG_OK;
}

/* ---- kernel lookup tables: one per templated family, naming exactly the instantiations the
 *      .hip files define (an entry without one would leave the library unloadable); a null
 *      entry is a case no kernel exists for ---- */
typedef void (*SgHistFn)(SgStackParams, const int *, const int4 *, unsigned int *, unsigned int *);
typedef void (*SgSortedFn)(SgStackParams, const unsigned int *, const unsigned int *);
typedef void (*SgReduce3Fn)(SgStackParams, const int *, const int *);
typedef void (*SgLinfitFn)(SgStackParams, unsigned int *, unsigned int *);
typedef void (*SgReplayFn)(SgStackParams);

/* k_stack_hist<REJ, NORM>: rows REJ = 1 PERCENTILE, 2 SIGMA, 3 SIGMEDIAN, 4 WINSORIZED, 8 stack_median */
static constexpr int SG_HIST_REJ[5] = {1, 2, 3, 4, 8};
#define SG_HIST_ROW(R) {k_stack_hist<R, 0>, k_stack_hist<R, 1>, k_stack_hist<R, 2>, k_stack_hist<R, 3>}
static constexpr SgHistFn SG_HIST_KERNELS[5][4] = {	/* [REJ row][NORM] */
	SG_HIST_ROW(1), SG_HIST_ROW(2), SG_HIST_ROW(3), SG_HIST_ROW(4), SG_HIST_ROW(8)};
#undef SG_HIST_ROW

#define SG_SORTED_ROW(R) {k_stack_sorted<R, false>, k_stack_sorted<R, true>}
static constexpr SgSortedFn SG_SORTED_KERNELS[5][2] = {	/* [log2 NREG][LISTED] */
	SG_SORTED_ROW(1), SG_SORTED_ROW(2), SG_SORTED_ROW(4), SG_SORTED_ROW(8), SG_SORTED_ROW(16)};
#undef SG_SORTED_ROW

#define SG_R3_ROW(M) {k_stack_reduce3<M, 1>, k_stack_reduce3<M, 2>, k_stack_reduce3<M, 4>}
static constexpr SgReduce3Fn SG_REDUCE3_KERNELS[5][3] = {	/* [M][log2 SEG] */
	SG_R3_ROW(0), SG_R3_ROW(1), SG_R3_ROW(2), SG_R3_ROW(3), SG_R3_ROW(4)};
#undef SG_R3_ROW

static constexpr SgLinfitFn SG_LINFIT_KERNELS[2][3] = {	/* [KM / 16][log2 (NW / 4)] */
	{k_stack_linfit<8, 4>, k_stack_linfit<8, 8>, k_stack_linfit<8, 16>},
	{k_stack_linfit<16, 4>, k_stack_linfit<16, 8>, nullptr}};

static constexpr SgReplayFn SG_REPLAY_KERNELS[2] = {k_stack_replay<512>, k_stack_replay<SG_REPLAY_MAXN>};	/* [N > 512] */

static int log2_index(int v, int n) {	/* i with v == 1 << i below n, else -1 */
	for (int i = 0; i < n; i++)
		if (v == 1 << i)
			return i;
	return -1;
}

static const void *hist_kernel(const SgStackPlan &pl) {
	for (int r = 0; r < 5; r++)
		if (SG_HIST_REJ[r] == pl.rj && pl.norm >= 0 && pl.norm < 4)
			return (const void *)SG_HIST_KERNELS[r][pl.norm];
	return nullptr;
}

static const void *linfit_kernel(const SgStackPlan &pl) {
	const int w = log2_index(pl.nw / 4, 3);
	return (pl.km == 8 || pl.km == 16) && w >= 0 ? (const void *)SG_LINFIT_KERNELS[pl.km / 16][w] : nullptr;
}

static hipError_t launch_sorted(int nreg, bool listed, dim3 grid, size_t lds, hipStream_t s, const SgStackParams &p,
		const unsigned int *list, const unsigned int *list_count) {
	const int r = log2_index(nreg, 5);
	if (r < 0)
		return hipErrorInvalidValue;
	const void *kf = (const void *)SG_SORTED_KERNELS[r][listed ? 1 : 0];
	(void)hipFuncSetAttribute(kf, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
	void *args[] = {(void *)&p, &list, &list_count};
	return hipLaunchKernel(kf, grid, dim3(SG_SORT_THREADS), args, lds, s);
}


/* SUM over row bands streamed by the host-pull path: the raw sums and the maximum carry
 * across the band calls, the scaling runs once after the last band */
enum { SUM_WHOLE = 0, SUM_FIRST_BAND = 1, SUM_MID_BAND = 2, SUM_LAST_BAND = 3 };

/* counter block of one slot: rejection shards (SG_CTR_REJB), then the flag words below */
static const size_t SG_CTRB = SG_CTR_REJB + 128;
/* host-mapped slot k_ctr_finalize writes: rejection sums at 0, the flag words at 64 */
static const size_t SG_CTR_HOSTB = 256;
/* the flag words (unsigned int) of a counter block, on the device and in the host copy */
enum SgFlagWord {
	SG_FL_SLOW = 0,		/* flag count: pixels queued for the replay / literal kernels */
	SG_FL_WALK_FAULT = 1,	/* a stale-state chain needs rows that are not resident */
	SG_FL_REDO = 2,		/* redo count of the histogram / linfit kernels */
	SG_FL_COMPACT = 3,	/* compact columns taken */
	SG_FL_LOOP_FAULT = 4,	/* a SIGMEDIAN pixel's reference loop never ends */
	SG_FL_VERDICT = 7,	/* k_norm_fma_check's load verdict */
	SG_FL_SUM_MAX = 16	/* SUM maximum, words 16 and 17 as one little-endian 64-bit value (byte 64: kept across
				 * the bands of a streamed SUM); the uint32_t kernels write word 16 alone, 17 stays 0 */
};
static unsigned int *flag_words(void *ctr_block) {
	return (unsigned int *)((char *)ctr_block + SG_CTR_REJB);
}

/*
 * wait for the call queued in counter slot `slot` and take its results: faults, the rejection
 * counters (rej, may be null), the SUM maximum, the call's statistics (published to the context)
 */
static int stack_fold(sg_ctx *ctx, SgDevice &dv, int slot, uint64_t rej[3][2], uint64_t *maxim_out, bool sync) {
	HIPCHK(hipEventSynchronize(dv.cev[slot][2]));
	dv.pend[slot] = false;
	dv.sl[slot].stage_pending = false;	/* the input copy ran before this call's kernels */
	const char *h = (const char *)dv.ctr_h + (size_t)slot * SG_CTR_HOSTB;
	const unsigned int *fl = (const unsigned int *)(h + 64);
	sg_stack_stats &st = dv.pstats[slot];
	float ms = 0.f, ms2 = 0.f;
	HIPCHK(hipEventElapsedTime(&ms, dv.cev[slot][0], dv.cev[slot][1]));
	HIPCHK(hipEventElapsedTime(&ms2, dv.cev[slot][0], dv.cev[slot][2]));
	st.kernel_ms = ms;
	st.total_ms = ms2;
	st.slow_pixels = fl[SG_FL_SLOW];
	if (st.path == 1)
		st.chain_pixels = fl[SG_FL_REDO];
	st.compact_pixels = std::min<uint64_t>(fl[SG_FL_COMPACT], st.compact_pixels);	/* pstats holds the capacity */
	if (st.norm_fma > 0)	/* k_norm_fma_check's verdict, read back beside the counters (the launch set the best allowed) */
		st.norm_fma = st.norm_fma == 2 && !(fl[SG_FL_VERDICT] & 2u) ? 2 : (fl[SG_FL_VERDICT] & 1u) ? 0 : 1;
	if (sync) {	/* the calling stack_device_core publishes dv.stats when it returns */
		dv.stats = st;
	} else {
		std::lock_guard<std::mutex> lk(ctx->mu);
		ctx->stats = st;
	}
	if (fl[SG_FL_LOOP_FAULT])
		return set_err(ctx, SG_ERR_GENERIC, "SIGMEDIAN: the reference's clipping loop never ends for some pixel "
				"(a pass replaces samples by the values they already hold, stacking.c:1696-1709)%s%.0ld", "", 0);
	if (fl[SG_FL_WALK_FAULT])
		return set_err(ctx, SG_ERR_WALK, "a first-pass early break needs the stale rejected[] of a pixel "
				"whose frame rows are not resident; make the full frames resident%s%.0ld", "", 0);
	if (rej) {
		const unsigned long long *sums = (const unsigned long long *)h;	/* k_ctr_finalize's */
		for (int c = 0; c < 3; c++) {
			rej[c][0] = sums[c * 2];
			rej[c][1] = sums[c * 2 + 1];
		}
	}
	if (maxim_out)
		*maxim_out = dv.pend_sum_read[slot] ? (uint64_t)fl[SG_FL_SUM_MAX] | (uint64_t)fl[SG_FL_SUM_MAX + 1] << 32 : 0;
	return SG_OK;
}

/* fold a pending async call into the device's accumulators (sg_stack_collect returns them) */
static void stack_fold_acc(sg_ctx *ctx, SgDevice &dv, int slot) {
	uint64_t r[3][2], mx = 0;
	const int rc = stack_fold(ctx, dv, slot, r, &mx, false);
	if (rc) {
		if (!dv.acc_rc)
			dv.acc_rc = rc == SG_ERR_WALK ? SG_ERR_GENERIC : rc;
		return;
	}
	for (int c = 0; c < 3; c++) {
		dv.acc_rej[c][0] += r[c][0];
		dv.acc_rej[c][1] += r[c][1];
	}
	dv.acc_max = std::max<uint64_t>(dv.acc_max, mx);
}

/* ---- the launch step of a stacking call: everything that touches the device, driven by the
 *      plan (sg_stack_plan.hpp) alone ---- */
struct StackCall {
	sg_ctx *ctx;
	SgDevice *dv;
	int slot;		/* counter slot and its buffers */
	SgSlot *sb;
	hipStream_t s, ts;	/* the call's stream; the stream of everything after the main kernel */
	SgStackParams p;
	SgChainTables ct;
	unsigned int *fl;	/* the slot's flag words on the device */
	unsigned int *redo_list;
};

/* the counter slot (and its buffers): a synchronous call uses slot 0 (a streamed SUM keeps its
 * maximum there), an async call the free slot, folding the older pending call when both are taken */
static int choose_slot(sg_ctx *ctx, SgDevice &dv, bool async) {
	if (!async) {
		if (dv.pend[0])
			stack_fold_acc(ctx, dv, 0);
		return 0;
	}
	if (dv.pend[0] && dv.pend[1])
		stack_fold_acc(ctx, dv, dv.pend_seq[0] < dv.pend_seq[1] ? 0 : 1);
	return dv.pend[0] ? 1 : 0;
}

/* counters: rejection shards, then the flag words; one memset, one read-back.  They are zero
 * when the slot's last call finished (k_ctr_finalize); a fresh or failed slot is cleared here
 * (SUM keeps its maximum across the bands of a streamed sum) */
static int prepare_counters(StackCall &c, const SgStackPlan &pl, int sum_mode) {
	sg_ctx *ctx = c.ctx;
	SgDevice &dv = *c.dv;
	const void *old_ctr = dv.ctr.p;
	HIPCHK(ensure(dv.ctr, 2 * SG_CTRB));
	if (dv.ctr.p != old_ctr)
		dv.ctr_clean[0] = dv.ctr_clean[1] = false;
	if (!dv.ctr_h) {
		HIPCHK(hipHostMalloc(&dv.ctr_h, 2 * SG_CTR_HOSTB, hipHostMallocMapped | hipHostMallocCoherent));
		HIPCHK(hipHostGetDevicePointer((void **)&dv.ctr_hd, dv.ctr_h, 0));
	}
	char *cblk = (char *)dv.ctr.p + (size_t)c.slot * SG_CTRB;
	c.fl = flag_words(cblk);
	const bool clear_max = sum_mode == SUM_WHOLE || sum_mode == SUM_FIRST_BAND;
	if (!dv.ctr_clean[c.slot])
		HIPCHK(hipMemsetAsync(cblk, 0, clear_max ? SG_CTRB : SG_CTR_REJB + SG_FL_SUM_MAX * sizeof(unsigned int), c.s));
	else if (clear_max && pl.sum)
		HIPCHK(hipMemsetAsync(c.fl + SG_FL_SUM_MAX, 0, 2 * sizeof(unsigned int), c.s));
	dv.ctr_clean[c.slot] = false;
	c.p.rej = (unsigned long long *)cblk;
	c.p.flag_count = c.fl + SG_FL_SLOW;
	c.p.walk_fault = c.fl + SG_FL_WALK_FAULT;
	c.p.loop_fault = c.fl + SG_FL_LOOP_FAULT;
	c.p.maxim = c.fl + SG_FL_SUM_MAX;
	return SG_OK;
}

/* the slot's buffers of a rejection / median stack, grown to the plan's sizes */
static int prepare_rejection_buffers(StackCall &c, const SgStackPlan &pl) {
	sg_ctx *ctx = c.ctx;
	SgSlot &sb = *c.sb;
	SgStackParams &p = c.p;
	HIPCHK(ensure(sb.flag_list, sizeof(unsigned int) * pl.npix_launch));
	/* pixel classes carry this call's epoch (sg_flag_get): no per-call clear; the map is
	 * cleared when it is new or the 31 epochs wrap */
	const void *old_map = sb.flag_map.p;
	HIPCHK(ensure(sb.flag_map, pl.npix_img));
	if (sb.flag_map.p != old_map || sb.flag_epoch <= 0 || sb.flag_epoch >= 31) {
		HIPCHK(hipMemsetAsync(sb.flag_map.p, 0, sb.flag_map.size, c.s));
		sb.flag_epoch = 0;
	}
	p.flag_epoch = (unsigned int)++sb.flag_epoch;
	p.flag_list = (unsigned int *)sb.flag_list.p;
	p.flag_cap = (unsigned int)pl.npix_launch;
	p.flag_map = (uint8_t *)sb.flag_map.p;
	HIPCHK(ensure(sb.scratch, pl.scratch_bytes));
	if (pl.linfit_tables) {
		HIPCHK(ensure(sb.lin_tab, sizeof(double) * 2 * ((size_t)pl.N + 1)));
		p.linfit_tab = (const double *)sb.lin_tab.p;
	}
	if (pl.redo != SG_REDO_NONE) {
		HIPCHK(ensure(sb.redo, sizeof(unsigned int) * (pl.npix_launch + 16)));
		c.redo_list = (unsigned int *)sb.redo.p + 16;
	}
	if (pl.compact) {
		HIPCHK(ensure(sb.cmp_cols, pl.cmp_cap * (size_t)pl.N * 2));
		HIPCHK(ensure(sb.cmp_list, pl.cmp_cap * sizeof(unsigned int)));
		p.cmp_cols = (uint16_t *)sb.cmp_cols.p;
		p.cmp_list = (unsigned int *)sb.cmp_list.p;
		p.cmp_count = c.fl + SG_FL_COMPACT;	/* cleared with the counters */
		p.cmp_cap = (unsigned int)pl.cmp_cap;
	}
	return SG_OK;
}

/* the call's inputs (shift table, normalisation coefficients, chain tables, border-row table)
 * reach the device in one copy: one pinned host block -> one device block; sets the kernels'
 * pointers into it */
static int stage_inputs(StackCall &c, const SgStackPlan &pl) {
	sg_ctx *ctx = c.ctx;
	SgSlot &sb = *c.sb;
	SgStackParams &p = c.p;
	const int N = pl.N, Npad = pl.Npad;
	const size_t b_sh = sizeof(int) * pl.sh.size(), o_nm = (b_sh + 255) & ~(size_t)255;
	const size_t b_nm = sizeof(double) * pl.nm.size(), o_tb = (o_nm + b_nm + 255) & ~(size_t)255;
	const size_t o_zt = (o_tb + sizeof(int) * pl.tables.size() + 255) & ~(size_t)255;
	const size_t tot = (o_zt + sizeof(int) * pl.ztab.size() + 15) & ~(size_t)15;
	if (sb.stage_pending) {	/* an earlier call's copy may still read the host block */
		HIPCHK(hipEventSynchronize(sb.stage_ev));
		sb.stage_pending = false;
	}
	if (sb.stage_h_size < tot) {
		if (sb.stage_h)
			(void)hipHostFree(sb.stage_h);
		sb.stage_h = nullptr;
		sb.stage_h_size = 0;
		/* coherent: the device reads it uncached, so no call sees an earlier call's inputs */
		HIPCHK(hipHostMalloc(&sb.stage_h, tot, hipHostMallocMapped | hipHostMallocCoherent));
		sb.stage_h_size = tot;
		HIPCHK(hipHostGetDevicePointer(&sb.stage_d, sb.stage_h, 0));
	}
	HIPCHK(ensure(sb.inb, tot));
	char *hb = (char *)sb.stage_h;
	memcpy(hb, pl.sh.data(), b_sh);
	if (b_nm)
		memcpy(hb + o_nm, pl.nm.data(), b_nm);
	if (!pl.tables.empty())
		memcpy(hb + o_tb, pl.tables.data(), sizeof(int) * pl.tables.size());
	if (!pl.ztab.empty())
		memcpy(hb + o_zt, pl.ztab.data(), sizeof(int) * pl.ztab.size());
	hipLaunchKernelGGL(k_stage_copy, dim3((unsigned)std::min<size_t>(64, (tot / 16 + 255) / 256)), dim3(256), 0, c.s,
			(uint4 *)sb.inb.p, (const uint4 *)sb.stage_d, (unsigned int)(tot / 16));
	HIPCHK(hipGetLastError());
	HIPCHK(hipEventRecord(sb.stage_ev, c.s));
	sb.stage_pending = true;
	const char *db = (const char *)sb.inb.p;
	p.hist_tab = (const int *)db;
	if (pl.use_shift) {
		p.shiftx = p.hist_tab + Npad + Npad / 2;
		p.shifty = p.shiftx + N;
	}
	if (pl.normalize) {
		p.offset = (const double *)(db + o_nm);
		p.mul = p.offset + N;
		p.scale = p.offset + 2 * N;
		p.hist_norm = p.offset + 3 * N;
	}
	p.ztab = pl.ztab.empty() ? nullptr : (const int *)(db + o_zt);
	memset(&c.ct, 0, sizeof c.ct);
	if (!pl.tables.empty()) {
		const int *tb = (const int *)(db + o_tb);
		c.ct.nblocks = pl.nblocks;
		c.ct.blk_of_row = tb;
		c.ct.blk_channel = tb + (size_t)pl.C * pl.H;
		c.ct.blk_start = c.ct.blk_channel + pl.nblocks;
		c.ct.blk_end = c.ct.blk_start + pl.nblocks;
		c.ct.blk_first = c.ct.blk_end + pl.nblocks;
	}
	return SG_OK;
}

/* everything after the main kernel runs on ts: the call's stream, or the device's tail stream
 * for an async call whose result is wanted at sg_stack_collect only (it then overlaps the
 * next call's main kernel, which uses the other slot's buffers) */
static int to_tail(StackCall &c, const SgStackPlan &pl, bool async) {
	sg_ctx *ctx = c.ctx;
	SgDevice &dv = *c.dv;
	if (!(async && pl.result_at_collect))
		return SG_OK;
	if (!dv.tail) {
		HIPCHK(hipStreamCreateWithFlags(&dv.tail, hipStreamNonBlocking));
		HIPCHK(hipEventCreateWithFlags(&dv.tail_ev, hipEventDisableTiming));
		HIPCHK(hipEventCreateWithFlags(&dv.tail_done_ev, hipEventDisableTiming));
	}
	HIPCHK(hipEventRecord(dv.tail_ev, c.s));
	HIPCHK(hipStreamWaitEvent(dv.tail, dv.tail_ev, 0));
	c.ts = dv.tail;
	return SG_OK;
}

/* A/B (probe builds): report the resident histogram workgroups per CU */
static void report_hist_occupancy(const StackCall &c, const SgStackPlan &pl) {
	int per_cu = -1;
	(void)hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, (const void *)SG_HIST_KERNELS[1][0],
			sgh_block_threads(2), (size_t)pl.hist_ldspad);
	hipDeviceProp_t prop;
	(void)hipGetDeviceProperties(&prop, c.dv->id);
	fprintf(stderr, "k_stack_hist: %d workgroups/CU (lds/CU %zu, lds/block max %zu, pad %d)\n", per_cu,
			(size_t)prop.maxSharedMemoryPerMultiProcessor, (size_t)prop.sharedMemPerBlock, pl.hist_ldspad);
}

/* the main kernel of a rejection / median stack between the events cev[0] and cev[1] */
static int launch_rejection_main(StackCall &c, const SgStackPlan &pl) {
	sg_ctx *ctx = c.ctx;
	SgStackParams &p = c.p;
	hipEvent_t *cev = c.dv->cev[c.slot];
	unsigned int *redo_count = c.fl + SG_FL_REDO;	/* cleared with the counters */
	if (pl.linfit_tables) {
		hipLaunchKernelGGL(k_linfit_tables, dim3((pl.N + 64) / 64), dim3(64), 0, c.s, (double *)c.sb->lin_tab.p, pl.N);
		HIPCHK(hipGetLastError());
	}
	HIPCHK(hipEventRecord(cev[0], c.s));
	const dim3 grid(pl.main_grid[0]);
	if (pl.main == SG_MAIN_HIST) {
		if (SG_DBG(p) == 14)
			report_hist_occupancy(c, pl);
		if (pl.norm_check) {
			hipLaunchKernelGGL(k_norm_fma_check, dim3(16, (unsigned)pl.N), dim3(256), 0, c.s, (double *)p.hist_norm, pl.N,
					pl.Npad, pl.norm, c.fl + SG_FL_VERDICT);
			HIPCHK(hipGetLastError());
		}
		const void *kf = hist_kernel(pl);
		if (!kf)
			return set_err(ctx, SG_ERR_GENERIC, "no histogram kernel for this case%s%.0ld", "", 0);
		const int4 *norm_pairs = (const int4 *)p.hist_norm;
		void *args[] = {&p, &p.hist_tab, &norm_pairs, &redo_count, &c.redo_list};
		HIPCHK(hipLaunchKernel(kf, grid, dim3((unsigned)sgh_block_threads(pl.rj)), args, pl.main_lds, c.s));
	} else if (pl.main == SG_MAIN_LINFIT) {
		const void *kf = linfit_kernel(pl);
		if (!kf)
			return set_err(ctx, SG_ERR_GENERIC, "no histogram kernel for this case%s%.0ld", "", 0);
		HIPCHK(hipFuncSetAttribute(kf, hipFuncAttributeMaxDynamicSharedMemorySize, (int)pl.main_lds));
		void *args[] = {&p, &redo_count, &c.redo_list};
		HIPCHK(hipLaunchKernel(kf, grid, dim3(pl.main_threads), args, pl.main_lds, c.s));
	} else if (pl.main == SG_MAIN_SORTED) {
		HIPCHK(launch_sorted(pl.nreg, false, grid, pl.sorted_lds, c.s, p, nullptr, nullptr));
	} else {
		hipLaunchKernelGGL(k_list_all, grid, dim3(pl.main_threads), 0, c.s, p);
		HIPCHK(hipGetLastError());
	}
	HIPCHK(hipEventRecord(cev[1], c.s));
	return SG_OK;
}

/* the compact columns and the redo pixels of the histogram / linfit kernels, routed on the
 * device (SgRedoRoute) */
static int launch_redo(StackCall &c, const SgStackPlan &pl) {
	sg_ctx *ctx = c.ctx;
	SgStackParams &p = c.p;
	unsigned int *redo_count = c.fl + SG_FL_REDO;
	const dim3 lgrid(SG_LIST_GRID);
	if (pl.compact) {
		/* the compact columns, any count up to the capacity (grid-stride) */
		SgStackParams q = p;
		q.cmp_src = p.cmp_cols;
		HIPCHK(launch_sorted(pl.nreg, true, lgrid, pl.sorted_lds, c.ts, q, p.cmp_list, p.cmp_count));
	}
	if (pl.redo == SG_REDO_REPLAY_THEN_SORTED) {
		SgStackParams q = p;
		q.list_minn = pl.list_minn;	/* idle unless the list is longer */
		HIPCHK(launch_sorted(pl.nreg, true, lgrid, pl.sorted_lds, c.ts, q, c.redo_list, redo_count));
		p.rp_list = c.redo_list;
		p.rp_count = redo_count;
		p.rp_maxn = pl.rp_maxn;
	} else if (pl.redo == SG_REDO_SORTED) {
		HIPCHK(launch_sorted(pl.nreg, true, lgrid, pl.sorted_lds, c.ts, p, c.redo_list, redo_count));
	} else if (pl.redo == SG_REDO_TO_LITERAL) {
		hipLaunchKernelGGL(k_redo_to_literal, dim3(64), dim3(256), 0, c.ts, p, (const unsigned int *)c.redo_list,
				(const unsigned int *)redo_count, 0xFFFFFFFFu);
		HIPCHK(hipGetLastError());
	}
	return SG_OK;
}

/* exact wave-per-pixel replay of queued SIGMA / WINSORIZED pixels, then the literal path for
 * what remains: two phases, grids read the count on the device */
static int launch_replay_literal(StackCall &c, const SgStackPlan &pl) {
	sg_ctx *ctx = c.ctx;
	if (pl.replay_nm) {
		void *args[] = {&c.p};
		HIPCHK(hipLaunchKernel((const void *)SG_REPLAY_KERNELS[pl.replay_nm > 512 ? 1 : 0], dim3(2048),
				dim3(64 * SG_REPLAY_WAVES), args, 0, c.ts));
	}
	for (int phase = 1; phase <= 2; phase++) {
		hipLaunchKernelGGL(k_stack_literal, dim3(pl.lit_threads / 64), dim3(64), 0, c.ts, c.p, c.ct, 0u,
				(uint8_t *)c.sb->scratch.p, phase);
		HIPCHK(hipGetLastError());
	}
	return SG_OK;
}

/* SUM / MEAN without rejection / MAX / MIN: the reduce kernel and SUM's scaling */
static int launch_reduce(StackCall &c, const SgStackPlan &pl, int sum_mode, sg_stack_stats &st) {
	sg_ctx *ctx = c.ctx;
	SgDevice &dv = *c.dv;
	SgStackParams &p = c.p;
	if (pl.sum) {
		HIPCHK(ensure(dv.sum_buf, (pl.wide ? sizeof(unsigned long long) : sizeof(uint32_t)) * pl.npix_img));
		p.sum_buf = (uint32_t *)dv.sum_buf.p;
	}
	const dim3 grid(pl.main_grid[0], pl.main_grid[1], pl.main_grid[2]);
	HIPCHK(hipEventRecord(dv.cev[c.slot][0], c.s));
	if (pl.main == SG_MAIN_REDUCE_WIDE) {
		hipLaunchKernelGGL(k_stack_reduce_wide, grid, dim3(pl.main_threads), 0, c.s, p);
	} else if (pl.main == SG_MAIN_REDUCE3) {
		const int g = log2_index(pl.seg, 3);
		if (g < 0 || pl.m < 0 || pl.m > 4)
			return set_err(ctx, SG_ERR_GENERIC, "no reduce kernel for this case%s%.0ld", "", 0);
		void *args[] = {&p, &p.hist_tab, &p.shifty};
		HIPCHK(hipLaunchKernel((const void *)SG_REDUCE3_KERNELS[pl.m][g], grid, dim3(pl.main_threads), args, 0, c.s));
	} else if (pl.main == SG_MAIN_REDUCE2) {
		hipLaunchKernelGGL(k_stack_reduce2, grid, dim3(pl.main_threads), 0, c.s, p);
	} else {
		hipLaunchKernelGGL(k_stack_reduce, grid, dim3(pl.main_threads), 0, c.s, p);
	}
	HIPCHK(hipGetLastError());
	HIPCHK(hipEventRecord(dv.cev[c.slot][1], c.s));
	if (pl.sum && (sum_mode == SUM_WHOLE || sum_mode == SUM_LAST_BAND)) {
		/* the 65535/max scaling (:328-342) needs the maximum over the whole image: a
		 * streamed sequence finalises every row once its last band is summed */
		SgStackParams pf = p;
		dim3 gf(pl.fin_grid_x, (unsigned)pl.nrows, (unsigned)pl.C);
		if (sum_mode == SUM_LAST_BAND) {
			pf.row_begin = 0;
			pf.row_end = pl.H;
			gf.y = pl.H;
		}
		hipLaunchKernelGGL(pl.wide ? k_sum_finalize_wide : k_sum_finalize, gf, dim3(256), 0, c.s, pf);
		HIPCHK(hipGetLastError());
		st.launches++;
	}
	return SG_OK;
}

/* the counters back to the host: queued; a synchronous call folds them at once, an async one
 * when its slot is needed again or at sg_stack_collect */
static int finalize_counters(StackCall &c, const SgStackPlan &pl, const sg_stack_stats &st) {
	sg_ctx *ctx = c.ctx;
	SgDevice &dv = *c.dv;
	if (SG_DBG(c.p) == 12)
		sg_dbg_why_dump(c.ts);
	hipLaunchKernelGGL(k_ctr_finalize, dim3(1), dim3(256), 0, c.ts, (unsigned long long *)c.p.rej,
			dv.ctr_hd + (size_t)c.slot * (SG_CTR_HOSTB / sizeof(unsigned long long)));
	HIPCHK(hipGetLastError());
	dv.ctr_clean[c.slot] = true;
	HIPCHK(hipEventRecord(dv.cev[c.slot][2], c.ts));
	dv.pend_sum_read[c.slot] = pl.sum;
	dv.pstats[c.slot] = st;
	dv.pend[c.slot] = true;
	dv.pend_seq[c.slot] = ++dv.seq;
	return SG_OK;
}

/* every launch of a planned call, in order */
static int launch_stack(StackCall &c, const SgStackPlan &pl, int sum_mode, bool async, sg_stack_stats &st) {
	if (int rc = prepare_counters(c, pl, sum_mode))
		return rc;
	/* the capacities of the compact and export lists; clamped to the counts when folded */
	st.path = pl.path;
	st.launches = pl.launches;
	st.main_kernel_blocks = pl.main_kernel_blocks;
	st.compact_pixels = pl.compact ? pl.cmp_cap : 0;
	st.norm_fma = pl.norm_fma;
	if (!pl.rejection_family) {
		if (int rc = stage_inputs(c, pl))
			return rc;
		if (int rc = launch_reduce(c, pl, sum_mode, st))
			return rc;
		return finalize_counters(c, pl, st);
	}
	if (int rc = prepare_rejection_buffers(c, pl))
		return rc;
	if (int rc = stage_inputs(c, pl))
		return rc;
	if (int rc = launch_rejection_main(c, pl))
		return rc;
	if (int rc = to_tail(c, pl, async))
		return rc;
	if (pl.redo != SG_REDO_NONE)
		if (int rc = launch_redo(c, pl))
			return rc;
	if (int rc = launch_replay_literal(c, pl))
		return rc;
	return finalize_counters(c, pl, st);
}

static int stack_device_core(sg_ctx *ctx, int dev_index, const sg_stack_desc *d,
		const uint16_t *d_frames, int64_t frame_stride, int64_t plane_stride, uint16_t *d_out,
		int row_begin, int row_end, uint64_t rej[3][2], uint64_t *maxim_out, void *stream, int sum_mode,
		bool async = false, int *slot_out = nullptr) {
	if (!ctx || !d || dev_index < 0 || dev_index >= (int)ctx->dev.size())
		return SG_ERR_GENERIC;
	SgDevice &dv = ctx->dev[dev_index];
	SgStackPlan pl;
	if (int rc = sg_stack_plan_args(d, row_begin, row_end, pl))
		return set_err(ctx, rc, "%s%.0ld", pl.err, 0);
	HIPCHK(hipSetDevice(dv.id));
	/* this call's statistics: the device's own record (one thread per device), published to the
	 * context when the call returns, whatever the outcome */
	sg_stack_stats &st = dv.stats;
	memset(&st, 0, sizeof st);
	struct Publish {
		sg_ctx *c;
		const sg_stack_stats &s;
		bool on;
		~Publish() {
			if (!on)	/* an async call's statistics are published when it is folded */
				return;
			std::lock_guard<std::mutex> lk(c->mu);
			c->stats = s;
		}
	} publish{ctx, st, !async};
	/* an error found by the plan is returned before any device work of the call */
	if (int rc = sg_stack_plan(d, row_begin, row_end, ctx->knobs, pl))
		return set_err(ctx, rc, "%s%.0ld", pl.err, 0);
	StackCall c;
	c.ctx = ctx;
	c.dv = &dv;
	c.slot = choose_slot(ctx, dv, async);
	c.sb = &dv.sl[c.slot];
	c.s = c.ts = stream ? (hipStream_t)stream : dv.stream;
	c.fl = c.redo_list = nullptr;
	sg_plan_params(pl, c.p);
	c.p.frames = d_frames;
	c.p.frame_stride = frame_stride;
	c.p.plane_stride = plane_stride;
	c.p.out = d_out;
	if (int rc = launch_stack(c, pl, sum_mode, async, st))
		return rc;
	if (slot_out)
		*slot_out = c.slot;
	if (async)
		return SG_OK;
	return stack_fold(ctx, dv, c.slot, rej, maxim_out, true);
}

extern "C" int sg_stack_u16_device(sg_ctx *ctx, int dev_index, const sg_stack_desc *d,
		const uint16_t *d_frames, int64_t frame_stride, int64_t plane_stride, uint16_t *d_out,
		int row_begin, int row_end, uint64_t rej[3][2], uint64_t *maxim_out, void *stream) {
	const int rc = stack_device_core(ctx, dev_index, d, d_frames, frame_stride, plane_stride, d_out, row_begin,
			row_end, rej, maxim_out, stream, SUM_WHOLE);
	return rc == SG_ERR_WALK ? SG_ERR_GENERIC : rc;
}

/* the same call queued without waiting: its counters come back with sg_stack_collect */
extern "C" int sg_stack_u16_device_async(sg_ctx *ctx, int dev_index, const sg_stack_desc *d,
		const uint16_t *d_frames, int64_t frame_stride, int64_t plane_stride, uint16_t *d_out,
		int row_begin, int row_end, void *stream) {
	const int rc = stack_device_core(ctx, dev_index, d, d_frames, frame_stride, plane_stride, d_out, row_begin,
			row_end, nullptr, nullptr, stream, SUM_WHOLE, true);
	return rc == SG_ERR_WALK ? SG_ERR_GENERIC : rc;
}

/* `stream` waits (on the device, the host does not block) for every tail kernel queued so far by
 * SG_STACK_RESULT_AT_COLLECT calls of this device slot: they read d_frames and write d_out after
 * the call's own stream has moved on, so a caller that refills d_frames or reuses d_out on its
 * stream before sg_stack_collect orders the refill behind this */
extern "C" int sg_stack_wait_tail(sg_ctx *ctx, int dev_index, void *stream) {
	if (!ctx || dev_index < 0 || dev_index >= (int)ctx->dev.size())
		return SG_ERR_GENERIC;
	SgDevice &dv = ctx->dev[(size_t)dev_index];
	if (!dv.tail)
		return SG_OK;
	HIPCHK(hipSetDevice(dv.id));
	HIPCHK(hipEventRecord(dv.tail_done_ev, dv.tail));
	HIPCHK(hipStreamWaitEvent(stream ? (hipStream_t)stream : dv.stream, dv.tail_done_ev, 0));
	return SG_OK;
}

extern "C" int sg_stack_collect(sg_ctx *ctx, int dev_index, uint64_t rej[3][2], uint64_t *maxim) {
	if (!ctx || dev_index < 0 || dev_index >= (int)ctx->dev.size())
		return SG_ERR_GENERIC;
	SgDevice &dv = ctx->dev[(size_t)dev_index];
	HIPCHK(hipSetDevice(dv.id));
	while (dv.pend[0] || dv.pend[1]) {
		const int slot = (dv.pend[0] && (!dv.pend[1] || dv.pend_seq[0] < dv.pend_seq[1])) ? 0 : 1;
		stack_fold_acc(ctx, dv, slot);
	}
	const int rc = dv.acc_rc;
	if (rej)
		for (int c = 0; c < 3; c++) {
			rej[c][0] = dv.acc_rej[c][0];
			rej[c][1] = dv.acc_rej[c][1];
		}
	if (maxim)
		*maxim = dv.acc_max;
	for (int c = 0; c < 3; c++)
		dv.acc_rej[c][0] = dv.acc_rej[c][1] = 0;
	dv.acc_max = 0;
	dv.acc_rc = 0;
	return rc;
}

/* device bytes a stack call holds besides the frames: the output image (2 B per sample),
 * flag list and redo list (4 + 4 B), flag map (1 B), SUM's sums (4 B, 8 B past SG_SUM_U32_MAXN
 * frames), the literal kernel's scratch, the readers' staging and the small tables */
static size_t fixed_device_bytes(int N, int W, int H, int C) {
	const size_t npix = (size_t)C * H * W;
	return npix * (N > SG_SUM_U32_MAXN ? 19 : 15) + lit_scratch_bytes(N) + ((size_t)4 << 20) +
		(size_t)SG_PULL_READERS * 2 * SG_PULL_CHUNK_BYTES;
}

/* HBM the host-pull path may fill with frames on one device: SG_HOST_BUDGET_BYTES (tests: the
 * frame budget itself), else 85 % of the free device memory (plus what the context already holds
 * for frames) less the call's other buffers, split between the context slots that share the card */
static size_t host_budget(const sg_ctx *ctx, SgDevice &dv, int N, int W, int H, int C) {
	if (ctx->knobs.host_budget > 0)
		return (size_t)ctx->knobs.host_budget;
	size_t fr = 0, tot = 0;
	if (hipMemGetInfo(&fr, &tot) != hipSuccess)
		return 0;
	const size_t b = (size_t)((double)(fr + dv.frames.size + dv.out.size) * 0.85) / (size_t)std::max(1, dv.shared);
	const size_t fixed = fixed_device_bytes(N, W, H, C);
	return b > fixed ? b - fixed : 0;
}

/* state shared by the device threads and their readers of one sg_stack_u16 call */
struct PullCall {
	const sg_stack_desc *d;
	sg_read_region_fn pull;
	void *user;
	sg_should_continue_fn cont;
	void *cont_user;
	int sy_min, sy_max;
	bool multi;			/* more than one device: SUM scales after every device's band */
	std::mutex cont_mu;		/* the caller's get_thread_run is asked from one thread at a time */
	std::atomic<int> stop{0};	/* a reader failed or the caller cancelled: every thread winds down */
	bool keep_going() {
		if (stop.load())
			return false;
		if (!cont)
			return true;
		std::lock_guard<std::mutex> lk(cont_mu);
		if (stop.load())
			return false;
		if (!cont(cont_user)) {
			stop = 1;
			return false;
		}
		return true;
	}
};

static int ensure_readers(sg_ctx *ctx, SgDevice &dv, int nreaders, size_t elems) {
	if ((int)dv.readers.size() < nreaders)
		dv.readers.resize((size_t)nreaders);
	for (int r = 0; r < nreaders; r++) {
		SgReader &rd = dv.readers[(size_t)r];
		if (!rd.stream) {
			HIPCHK(hipStreamCreateWithFlags(&rd.stream, hipStreamNonBlocking));
			for (int k = 0; k < 2; k++)
				HIPCHK(hipEventCreateWithFlags(&rd.ev[k], hipEventDisableTiming));
		}
		if (rd.cap < elems) {
			for (int k = 0; k < 2; k++) {
				if (rd.used[k])
					HIPCHK(hipEventSynchronize(rd.ev[k]));
				rd.used[k] = false;
				if (rd.pin[k])
					(void)hipHostFree(rd.pin[k]);
				if (rd.dstage[k])
					(void)hipFree(rd.dstage[k]);
				rd.pin[k] = rd.dstage[k] = nullptr;
			}
			rd.cap = 0;
			for (int k = 0; k < 2; k++) {
				HIPCHK(hipHostMalloc((void **)&rd.pin[k], elems * sizeof(uint16_t)));
				HIPCHK(hipMalloc((void **)&rd.dstage[k], elems * sizeof(uint16_t)));
			}
			rd.cap = elems;
		}
	}
	return SG_OK;
}

/*
 * One band of frame rows onto one device: memory rows [lo, lo + nres) of every frame and
 * channel into `frames` (plane (i C + c) at (i C + c) nres W).  Like the reference's OpenMP
 * team reading its blocks (stacking.c:1513-1591, seq_opened_read_region under per-file locks),
 * `nreaders` host threads pull frames i = r, r + R, ... in top-down row chunks of at most
 * SG_PULL_CHUNK_BYTES into their two pinned buffers (the reader refills one while the other is
 * in flight), copy each chunk on their own stream and flip it into place on the device.  The
 * caller's cancellation is polled once per frame, as get_thread_run() is per frame read
 * (:1539).  Returns once every chunk has landed.
 */
static int pull_band(sg_ctx *ctx, SgDevice &dv, PullCall &pc, int nreaders, uint16_t *frames, int lo, int nres) {
	const sg_stack_desc *d = pc.d;
	const int N = d->nb_frames, W = d->width, H = d->height, C = d->nb_layers;
	const int chunk = (int)std::max<size_t>(1, SG_PULL_CHUNK_BYTES / ((size_t)W * sizeof(uint16_t)));
	const size_t bplane = (size_t)nres * W;
	std::atomic<int> rc{SG_OK};
	auto fail = [&](int code) {
		int expect = SG_OK;
		rc.compare_exchange_strong(expect, code);
		pc.stop = 1;
	};
	auto work = [&](int r) {
		SgReader &rd = dv.readers[(size_t)r];
		if (hipSetDevice(dv.id) != hipSuccess)
			return fail(set_err(ctx, SG_ERR_DEVICE, "hipSetDevice failed in a reader%s%ld", "", dv.id));
		int k = 0;
		for (int i = r; i < N; i += nreaders) {
			if (!pc.keep_going())
				return fail(SG_ERR_GENERIC);	/* cancelled, or another thread failed */
			for (int c = 0; c < C; c++) {
				uint16_t *plane = frames + ((size_t)i * C + c) * bplane;
				for (int m0 = 0; m0 < nres; m0 += chunk) {
					const int h = std::min(chunk, nres - m0);
					if (rd.used[k] && hipEventSynchronize(rd.ev[k]) != hipSuccess)
						return fail(set_err(ctx, SG_ERR_DEVICE, "staging event failed%s%ld", "", i));
					/* memory rows lo + m0 .. lo + m0 + h - 1 as the top-down area the
					 * region reader takes (y = H - 1 - the highest memory row) */
					const sg_rect area = {0, H - lo - m0 - h, W, h};
					if (pc.pull(pc.user, c, i, rd.pin[k], &area) < 0)
						return fail(set_err(ctx, SG_ERR_READ, "could not read frame%s %ld", "", i));
					if (hipMemcpyAsync(rd.dstage[k], rd.pin[k], (size_t)h * W * sizeof(uint16_t), hipMemcpyHostToDevice,
							rd.stream) != hipSuccess)
						return fail(set_err(ctx, SG_ERR_DEVICE, "upload failed for frame%s %ld", "", i));
					hipLaunchKernelGGL(k_flip_rows, dim3((unsigned)std::min(64, (W + 255) / 256), (unsigned)h), dim3(256), 0,
							rd.stream, (const uint16_t *)rd.dstage[k], plane + (size_t)m0 * W, W, h);
					if (hipGetLastError() != hipSuccess || hipEventRecord(rd.ev[k], rd.stream) != hipSuccess)
						return fail(set_err(ctx, SG_ERR_DEVICE, "flip launch failed for frame%s %ld", "", i));
					rd.used[k] = true;
					k ^= 1;
				}
			}
		}
	};
	std::vector<std::thread> th;
	int started = 1;
	for (int r = 1; r < nreaders; r++) {
		try {
			th.emplace_back(work, r);
			started++;
		} catch (...) {	/* no thread: the frames of the readers not started go unread -> fail */
			fail(set_err(ctx, SG_ERR_GENERIC, "could not start reader thread%s %ld", "", r));
			break;
		}
	}
	if (started == nreaders)
		work(0);
	for (std::thread &t : th)
		t.join();
	for (int r = 0; r < nreaders; r++)
		if (hipStreamSynchronize(dv.readers[(size_t)r].stream) != hipSuccess && rc.load() == SG_OK)
			fail(set_err(ctx, SG_ERR_DEVICE, "upload stream failed%s%ld", "", r));
	return rc.load();
}

/*
 * The rows [B, E) of the output on device g: banded under the device's HBM budget like the
 * reference's row blocks (stacking.c:1397-1476, sized from the memory budget :1903-1915); each
 * band's frame rows (the rows its shifts reach, :1544-1577) are pulled by the device's readers
 * and stacked with only those rows resident.  With two frame buffers (every method but SUM,
 * whose 65535/max scaling carries one maximum across the bands) band k + 1 is read while band k
 * stacks: the stack is queued without waiting (sg_stack_u16_device_async's path) and folded
 * once the next band has landed, as the reference's team reads blocks while other threads stack
 * theirs (:1513-1591).  The output rows stay in the device's dv.out (SUM of several devices:
 * raw sums, scaled once the maximum over every device is known).
 */
/* output rows per band (in: the rows wanted) and frame buffers under the device's budget */
static int pull_band_rows(sg_ctx *ctx, const sg_stack_desc *d, size_t budget, size_t row_bytes, int64_t halo,
		int &band, int &nbuf) {
	nbuf = 1;
	if ((size_t)band * row_bytes <= budget)
		return SG_OK;
	const int64_t fit = (int64_t)(budget / row_bytes) - halo;
	if (fit < 1)
		return set_err(ctx, SG_ERR_SIZE, "the sequence does not fit the device even one row at a "
				"time%s%.0ld", "", 0);
	band = (int)std::min<int64_t>(fit, band);
	/* several bands: two half-size buffers when a band of each still fits */
	const int64_t fit2 = (int64_t)(budget / 2 / row_bytes) - halo;
	if (d->method != SG_STACK_SUM && fit2 >= 1 && ctx->knobs.pull_overlap) {
		band = (int)std::min<int64_t>(fit2, band);
		nbuf = 2;
	}
	return SG_OK;
}

/* give up the band in flight (an error ends the call): wait for it, free its slot */
static void drain_pending(SgDevice &dv, int &slot) {
	if (slot < 0)
		return;
	(void)hipEventSynchronize(dv.cev[slot][2]);
	dv.pend[slot] = false;
	slot = -1;
}

static void add_rej(uint64_t rej[3][2], const uint64_t band[3][2]) {
	for (int c = 0; c < 3; c++) {
		rej[c][0] += band[c][0];
		rej[c][1] += band[c][1];
	}
}

static int pull_device(sg_ctx *ctx, int g, PullCall &pc, int B, int E, int nreaders, uint64_t rej[3][2],
		uint64_t *maxim) {
	SgDevice &dv = ctx->dev[(size_t)g];
	const sg_stack_desc *d = pc.d;
	const int N = d->nb_frames, W = d->width, H = d->height, C = d->nb_layers;
	HIPCHK(hipSetDevice(dv.id));
	const int64_t halo = std::min<int64_t>((int64_t)pc.sy_max - pc.sy_min, H);
	const size_t row_bytes = (size_t)N * C * W * sizeof(uint16_t);	/* one row of every frame */
	int band = E - B, nbuf = 1;
	if (int rc = pull_band_rows(ctx, d, host_budget(ctx, dv, N, W, H, C), row_bytes, halo, band, nbuf))
		return rc;
	const int64_t rows_cap = std::min<int64_t>(band + halo, H);
	const size_t buf_elems = (size_t)rows_cap * W * C * N;
	HIPCHK(ensure(dv.frames, nbuf * buf_elems * sizeof(uint16_t)));
	HIPCHK(ensure(dv.out, (size_t)W * H * C * sizeof(uint16_t)));
	const size_t chunk_elems = std::min<size_t>((size_t)rows_cap * W,
			std::max<size_t>(1, SG_PULL_CHUNK_BYTES / ((size_t)W * sizeof(uint16_t))) * W);
	if (int rc = ensure_readers(ctx, dv, nreaders, chunk_elems))
		return rc;
	for (int c = 0; c < 3; c++)
		rej[c][0] = rej[c][1] = 0;
	const bool banded = band < E - B || pc.multi;
	/* extra: rows above the band kept resident besides the halo.  A first-pass early break
	 * inherits the stale rejected[] of the previous pixel of the reference's OpenMP thread
	 * (stacking.c:1684), i.e. of the pixel one memory row up (rows run top-down inside a
	 * block); when that pixel lies above the band the core reports it (SG_ERR_WALK) and the
	 * band is retried narrower with more rows above it resident (same total rows) */
	int extra = 0;
	struct Pending {
		int slot, b, e, hi;
	} pend = {-1, 0, 0, 0};
	/* the band in flight: its counters, or a retry of it (the band start goes back to it) */
	auto fold = [&](int &b) -> int {
		uint64_t brej[3][2];
		const int rc = stack_fold(ctx, dv, pend.slot, brej, nullptr, true);
		const Pending pd = pend;
		pend.slot = -1;
		if (!pc.multi) {	/* one device: its folded band is the call's statistics (sg_get_last_stats) */
			std::lock_guard<std::mutex> lk(ctx->mu);
			ctx->stats = dv.stats;
		}
		if (rc == SG_ERR_WALK && pd.hi < H - 1 && pd.e - pd.b > 1) {
			extra = std::min(pd.e - pd.b - 1 + extra, extra ? 2 * extra : 4);
			b = pd.b;
			return 1;
		}
		if (rc)
			return rc == SG_ERR_WALK ? SG_ERR_GENERIC : rc;
		add_rej(rej, brej);
		return SG_OK;
	};
	int buf = 0;
	for (int b = B; b < E;) {
		const int e = std::min(E, b + std::max(1, band - extra));
		int lo = (int)std::max<int64_t>(0, (int64_t)b - pc.sy_max);
		int hi = (int)std::min<int64_t>(H - 1, (int64_t)e - 1 - pc.sy_min + extra);
		if (lo > hi)	/* every row of the band is shifted out of the frames: nothing is read */
			lo = hi = std::min(b, H - 1);
		const int nres = hi - lo + 1;
		const size_t bplane = (size_t)nres * W;
		uint16_t *fb = (uint16_t *)dv.frames.p + (size_t)buf * buf_elems;
		if (int rc = pull_band(ctx, dv, pc, nreaders, fb, lo, nres)) {
			drain_pending(dv, pend.slot);
			return rc;
		}
		if (pend.slot >= 0) {	/* the previous band stacked while this one was read */
			int bb = b;
			const int rc = fold(bb);
			if (rc < 0)
				return rc;
			if (rc == 1) {	/* retry it narrower: this band's rows are read again afterwards */
				b = bb;
				continue;
			}
		}
		sg_stack_desc bd = *d;
		bd.resident_rows[0] = lo;
		bd.resident_rows[1] = hi + 1;
		const int sum_mode = d->method != SG_STACK_SUM || !banded ? SUM_WHOLE
			: b == B ? SUM_FIRST_BAND : (!pc.multi && e == H) ? SUM_LAST_BAND : SUM_MID_BAND;
		/* base pointer biased so that memory row r of a frame plane sits at r*W */
		const uint16_t *base = fb - (ptrdiff_t)lo * W;
		if (nbuf == 2) {
			int slot = -1;
			if (int rc = stack_device_core(ctx, g, &bd, base, (int64_t)bplane * C, (int64_t)bplane,
					(uint16_t *)dv.out.p, b, e, nullptr, nullptr, dv.stream, sum_mode, true, &slot)) {
				drain_pending(dv, pend.slot);
				return rc == SG_ERR_WALK ? SG_ERR_GENERIC : rc;
			}
			pend = {slot, b, e, hi};
			buf ^= 1;
			b = e;
			if (b >= E) {	/* the last band: fold it here (a retry loops back) */
				const int rc = fold(b);
				if (rc < 0)
					return rc;
			}
			continue;
		}
		uint64_t brej[3][2];
		int rc = stack_device_core(ctx, g, &bd, base, (int64_t)bplane * C, (int64_t)bplane, (uint16_t *)dv.out.p, b,
				e, brej, maxim, dv.stream, sum_mode);
		if (rc == SG_ERR_WALK && hi < H - 1 && band - extra > 1) {
			extra = std::min(band - 1, extra ? 2 * extra : 4);
			continue;	/* same band start, narrower band, more rows above resident */
		}
		if (rc)
			return rc == SG_ERR_WALK ? SG_ERR_GENERIC : rc;
		add_rej(rej, brej);
		b = e;
	}
	return SG_OK;
}

/* SUM over several devices: the 65535/max scaling of stack_summing (:328-342) with the maximum
 * over the whole image, applied to device g's rows [B, E) of raw sums */
static int sum_finalize_rows(sg_ctx *ctx, int g, int W, int H, int C, int B, int E, uint64_t gmax, bool wide) {
	SgDevice &dv = ctx->dev[(size_t)g];
	HIPCHK(hipSetDevice(dv.id));
	SgStackParams p;
	memset(&p, 0, sizeof p);
	p.W = W;
	p.H = H;
	p.C = C;
	p.out = (uint16_t *)dv.out.p;
	p.sum_buf = (uint32_t *)dv.sum_buf.p;
	p.row_begin = B;
	p.row_end = E;
	p.maxim = flag_words(dv.ctr.p) + SG_FL_SUM_MAX;
	HIPCHK(hipMemcpyAsync(p.maxim, &gmax, sizeof gmax, hipMemcpyHostToDevice, dv.stream));
	hipLaunchKernelGGL(wide ? k_sum_finalize_wide : k_sum_finalize, dim3((unsigned)((W + 255) / 256), (unsigned)(E - B),
			(unsigned)C), dim3(256), 0, dv.stream, p);
	HIPCHK(hipGetLastError());
	HIPCHK(hipStreamSynchronize(dv.stream));
	return SG_OK;
}

/* a host-pull call's statistics over every device */
static void publish_multi_stats(sg_ctx *ctx, int G) {
	sg_stack_stats agg;
	memset(&agg, 0, sizeof agg);
	for (int g = 0; g < G; g++) {
		const sg_stack_stats &s = ctx->dev[(size_t)g].stats;
		agg.kernel_ms = std::max(agg.kernel_ms, s.kernel_ms);
		agg.total_ms = std::max(agg.total_ms, s.total_ms);
		agg.slow_pixels += s.slow_pixels;
		agg.chain_pixels += s.chain_pixels;
		agg.compact_pixels += s.compact_pixels;
		agg.norm_fma = std::max(agg.norm_fma, s.norm_fma);
		agg.launches += s.launches;
		agg.main_kernel_blocks += s.main_kernel_blocks;
		agg.path = s.path;
	}
	std::lock_guard<std::mutex> lk(ctx->mu);
	ctx->stats = agg;
}

/*
 * host-pull path: frames come through seq_opened_read_region-shaped callbacks.  Every device of
 * the context takes a contiguous share of the output rows (the reference's row blocks are the
 * natural shard) and is driven by its own host thread, whose readers pull and upload
 * that share's frame rows directly (no device relays another's data); each device's band is
 * copied back into `out`, the rejection counters are summed.
 */
extern "C" int sg_stack_u16(sg_ctx *ctx, const sg_stack_desc *d, sg_read_region_fn pull, void *user,
		sg_should_continue_fn cont, void *cont_user, uint16_t *out, uint64_t rej[3][2],
		uint64_t *maxim) {
	if (!ctx || !d || !pull || !out || ctx->dev.empty())
		return SG_ERR_GENERIC;
	const int N = d->nb_frames, W = d->width, H = d->height, C = d->nb_layers;
	if (N < 2)
		return set_err(ctx, SG_ERR_GENERIC, "select at least two frames%s (%ld)", "", N);
	if (W <= 0 || H <= 0 || C < 1 || C > 3)
		return SG_ERR_SIZE;
	PullCall pc;
	pc.d = d;
	pc.pull = pull;
	pc.user = user;
	pc.cont = cont;
	pc.cont_user = cont_user;
	/* frame rows a band reads: [b - sy_max, e - 1 - sy_min] */
	(void)sg_plan_shift_range(d, &pc.sy_min, &pc.sy_max);
	const int G = (int)std::min<size_t>(ctx->dev.size(), (size_t)H);
	pc.multi = G > 1;
	/* readers per device: the reference's team size (com.max_thread) shared between the
	 * devices, at least one, at most SG_PULL_READERS */
	const int team = d->max_thread > 0 ? d->max_thread : default_threads();
	const int nreaders = std::max(1, std::min(SG_PULL_READERS, team / G));
	std::vector<int> rb((size_t)G + 1);
	for (int g = 0; g <= G; g++)
		rb[(size_t)g] = (int)((int64_t)g * H / G);
	std::vector<int> rcs((size_t)G, SG_OK);
	std::vector<std::array<uint64_t, 6>> rj((size_t)G);
	std::vector<uint64_t> mx((size_t)G, 0);
	/* SUM over several devices scales with the maximum over all of them (after the join);
	 * every other result leaves its device from the device's own thread */
	const bool late_copy = d->method == SG_STACK_SUM && pc.multi;
	auto copy_out = [&](int g) -> int {
		SgDevice &dv = ctx->dev[(size_t)g];
		const int B = rb[(size_t)g], E = rb[(size_t)g + 1];
		HIPCHK(hipSetDevice(dv.id));
		for (int c = 0; c < C; c++) {
			const size_t o = ((size_t)c * H + B) * W;
			HIPCHK(hipMemcpy(out + o, (const uint16_t *)dv.out.p + o, (size_t)(E - B) * W * sizeof(uint16_t),
					hipMemcpyDeviceToHost));
		}
		return SG_OK;
	};
	auto run = [&](int g) {
		uint64_t r6[3][2];
		int r = pull_device(ctx, g, pc, rb[(size_t)g], rb[(size_t)g + 1], nreaders, r6, &mx[(size_t)g]);
		if (r == SG_OK && !late_copy)
			r = copy_out(g);
		rcs[(size_t)g] = r;
		if (r)
			pc.stop = 1;
		memcpy(rj[(size_t)g].data(), r6, sizeof r6);
	};
	{
		std::vector<std::thread> th;
		bool started = true;
		for (int g = 1; g < G; g++) {
			try {
				th.emplace_back(run, g);
			} catch (...) {
				rcs[(size_t)g] = set_err(ctx, SG_ERR_GENERIC, "could not start the thread of device slot%s %ld", "", g);
				pc.stop = 1;
				started = false;
				break;
			}
		}
		if (started)
			run(0);
		else
			rcs[0] = SG_ERR_GENERIC;
		for (std::thread &t : th)
			t.join();
	}
	/* a device's own failure wins over the stop (SG_ERR_GENERIC) it caused in the others;
	 * a cancellation alone is SG_ERR_GENERIC, as get_thread_run() going false is (-1) */
	int rc = SG_OK;
	for (int g = 0; g < G && rc == SG_OK; g++)
		if (rcs[(size_t)g] != SG_ERR_GENERIC)
			rc = rcs[(size_t)g];
	for (int g = 0; g < G && rc == SG_OK; g++)
		rc = rcs[(size_t)g];
	if (rc) {
		for (int g = 0; g < G; g++) {
			(void)hipSetDevice(ctx->dev[(size_t)g].id);
			(void)hipStreamSynchronize(ctx->dev[(size_t)g].stream);
		}
		return rc;
	}
	uint64_t gmax = 0;
	for (int g = 0; g < G; g++)
		gmax = std::max(gmax, mx[(size_t)g]);
	for (int g = 0; g < G && late_copy; g++) {
		if (int r = sum_finalize_rows(ctx, g, W, H, C, rb[(size_t)g], rb[(size_t)g + 1], gmax,
				sg_sum_wide(d->method, N)))
			return r;
		if (int r = copy_out(g))
			return r;
	}
	if (rej)
		for (int c = 0; c < 3; c++) {
			rej[c][0] = rej[c][1] = 0;
			for (int g = 0; g < G; g++) {
				rej[c][0] += rj[(size_t)g][(size_t)c * 2];
				rej[c][1] += rj[(size_t)g][(size_t)c * 2 + 1];
			}
		}
	if (maxim)
		*maxim = gmax;
	if (pc.multi)
		publish_multi_stats(ctx, G);
	return SG_OK;
}

extern "C" int sg_synth_fill_frames_device(sg_ctx *ctx, int dev_index, uint16_t *d_frames, int first_frame,
		int nframes, int nb_layers, int height, int width, int row_begin, int row_end, uint64_t seed,
		int maxshift, int64_t frame_stride, int64_t plane_stride, void *stream) {
	if (!ctx || dev_index < 0 || dev_index >= (int)ctx->dev.size() || first_frame < 0)
		return SG_ERR_GENERIC;
	SgDevice &dv = ctx->dev[dev_index];
	HIPCHK(hipSetDevice(dv.id));
	hipStream_t s = stream ? (hipStream_t)stream : dv.stream;
	hipLaunchKernelGGL(k_synth_fill, dim3(8192), dim3(256), 0, s, d_frames, first_frame, nframes, nb_layers,
			height, width, row_begin, row_end, seed, maxshift,
			frame_stride > 0 ? frame_stride : (int64_t)nb_layers * height * width,
			plane_stride > 0 ? plane_stride : (int64_t)height * width);
	HIPCHK(hipGetLastError());
	HIPCHK(hipStreamSynchronize(s));
	return SG_OK;
}

extern "C" int sg_synth_fill_device(sg_ctx *ctx, int dev_index, uint16_t *d_frames, int nframes,
		int nb_layers, int height, int width, int row_begin, int row_end, uint64_t seed,
		int maxshift, int64_t frame_stride, void *stream) {
	return sg_synth_fill_frames_device(ctx, dev_index, d_frames, 0, nframes, nb_layers, height, width, row_begin,
			row_end, seed, maxshift, frame_stride, 0, stream);
}
