/*
 * sg_seqpsf.hip - one-star registration on resident frames (include/sirilgpu.h, sg_seqpsf_u16*):
 * seqpsf's per-frame work, psf_get_minimisation of a rectangular selection with the angle fit.
 *
 *   - sgq_frame, the per-frame device function of both kernels, run by one workgroup: the box goes
 *     into LDS as u16 once; the non-zero median is a two-pass radix select over the LDS box (8 + 8
 *     bits, integer and exact); the first maximum of the 3x3-median-filtered box is a 64-bit ordered
 *     key reduction (value above, 2^32 - 1 - index below: 16384 pixels do not fit beside a 16-bit
 *     value in 32 bits); the two fits run sg_psf.h's solver in every thread on a workgroup-wide
 *     evaluator: pixels strided over the threads, a butterfly per wave, the waves' partial sums added
 *     in wave order through LDS.  Every thread holds the same bits, so the solver's branches, and the
 *     barriers inside the evaluator, are workgroup-uniform.
 *   - k_seqpsf_frames: ORIGINAL and REGISTERED framing, one workgroup per frame, the clamped areas
 *     from the plan's table.
 *   - k_seqpsf_chain: FOLLOW_STAR framing, one launch of one workgroup that walks the included frames
 *     in index order with the carried area in LDS; it stops at the first frame without a PSF and
 *     marks the rest SG_SEQPSF_NOT_RUN.  No host look between frames.
 */
#include <hip/hip_runtime.h>
#include <algorithm>
#include <vector>
#include "sg_ctx.hpp"
#include "sg_seqpsf_plan.hpp"

static_assert(SGQ_THREADS == 64 || SGQ_THREADS == 256 || SGQ_THREADS == 1024, "whole waves, at most 16");
static_assert(sizeof(sg_seqpsf_frame) % 8 == 0 && sizeof(SgSeqpsfItem) == 16, "record layouts");

struct SgSeqpsfParams {
	const uint16_t *img;
	int64_t frame_pitch, row_pitch;
	int W, H, w, h, nframes, fit_angle;
	unsigned lds_box;
	double norm, scale_x, scale_y;
	const SgSeqpsfItem *items;
	sg_seqpsf_frame *rec;
	int *carry;		/* [2]: the chain's carried area on return */
	int start_x, start_y;
};

/* a workgroup's LDS (sgq_lds_bytes) */
struct SgqLds {
	uint16_t *box;
	double *part;			/* [waves][SGQ_NSUM] */
	uint32_t *hist;			/* [SGQ_HIST] */
	unsigned long long *scal;	/* [16] */
	unsigned long long *wkey;	/* [waves] */
};
enum { SGQ_S_NGOOD = 0, SGQ_S_BIN = 1, SGQ_S_BEFORE = 2, SGQ_S_N65535 = 3, SGQ_S_AX = 8, SGQ_S_AY = 9, SGQ_S_STOP = 10 };

__device__ static inline SgqLds sgq_lds(unsigned char *base, unsigned lds_box, int waves) {
	SgqLds L;
	L.box = (uint16_t *)base;
	L.part = (double *)(base + lds_box);
	L.hist = (uint32_t *)(L.part + waves * SGQ_NSUM);
	L.scal = (unsigned long long *)(L.hist + SGQ_HIST);
	L.wkey = L.scal + 16;
	return L;
}

/* the lanes' values added in a fixed order; every lane receives the same bits (sgs_wave_sum) */
__device__ static inline double sgq_wave_sum(double v) {
#pragma unroll
	for (int o = 32; o >= 1; o >>= 1)
		v += __shfl_xor(v, o, 64);
	return v;
}

/* K per-thread values -> their sums over the workgroup in every thread: the wave butterflies, then
 * the waves' partial sums in wave order.  Called by all threads. */
template <int T, int K>
__device__ static inline void sgq_block_sum(double *v, double *part, int tid) {
	static_assert(K <= SGQ_NSUM, "the partials' row");
#pragma unroll
	for (int k = 0; k < K; k++)
		v[k] = sgq_wave_sum(v[k]);
	if (T > 64) {
		if ((tid & 63) == 0) {
#pragma unroll
			for (int k = 0; k < K; k++)
				part[(tid >> 6) * SGQ_NSUM + k] = v[k];
		}
		__syncthreads();
#pragma unroll
		for (int k = 0; k < K; k++) {
			double t = part[k];
			for (int wv = 1; wv < T / 64; wv++)
				t += part[wv * SGQ_NSUM + k];
			v[k] = t;
		}
		__syncthreads();	/* the partials are free again */
	}
}

/* the evaluator of sgp_lm over a box in LDS: pixel q = i * w + j belongs to thread q % T */
template <int T>
struct SgqEval {
	const uint16_t *box;
	double *part;
	int w, ne, tid;
	template <int NP>
	__device__ void full(const double *x, SgPsfSums<NP> &s) const {
		static_assert(sizeof(SgPsfSums<NP>) == (NP * (NP + 1) / 2 + NP + 1) * sizeof(double), "a plain row of doubles");
		sgp_sums_zero<NP>(s);
		const SgPsfModel<NP> m = sgp_model<NP>(x);
		for (int q = tid; q < ne; q += T) {
			const int i = q / w, j = q - i * w;
			sgp_pixel<NP>(x, m, (double)(j + 1), (double)(i + 1), (double)box[q], s);
		}
		sgq_block_sum<T, NP *(NP + 1) / 2 + NP + 1>(&s.a[0], part, tid);
	}
	template <int NP>
	__device__ double resid(const double *x) const {
		const SgPsfModel<NP> m = sgp_model<NP>(x);
		double ff = 0.;
		for (int q = tid; q < ne; q += T) {
			const int i = q / w, j = q - i * w;
			const double r = sgp_resid<NP>(x, m, (double)(j + 1), (double)(i + 1), (double)box[q]);
			ff += r * r;
		}
		sgq_block_sum<T, 1>(&ff, part, tid);
		return ff;
	}
	__device__ double flux(double B) const {
		double t = 0.;
		for (int q = tid; q < ne; q += T)
			t += (double)box[q] - B;
		sgq_block_sum<T, 1>(&t, part, tid);
		return t;
	}
};

/* one pass of the radix select: the bins of (v >> shift) & 255 over the non-zero values below 65535
 * whose upper bits match `prefix` (shift = 8: all of them), then thread 0 walks the bins from
 * `before` until twice the running count exceeds ngood.  L.scal[SGQ_S_BIN] = the bin or 256,
 * [SGQ_S_BEFORE] = the count before it.  Ends synchronised. */
template <int T>
__device__ static inline void sgq_select_pass(const SgqLds &L, int ne, int tid, int shift, unsigned prefix) {
	for (int b = tid; b < SGQ_HIST; b += T)
		L.hist[b] = 0;
	if (tid == 0 && shift == 8)
		L.scal[SGQ_S_N65535] = 0;
	__syncthreads();
	unsigned n65535 = 0;
	for (int q = tid; q < ne; q += T) {
		const unsigned v = L.box[q];
		if (v == 65535u)
			n65535++;
		else if (v != 0 && (shift == 8 || (v >> 8) == prefix))
			atomicAdd(&L.hist[(v >> shift) & 255u], 1u);
	}
	if (shift == 8 && n65535)
		atomicAdd(&L.scal[SGQ_S_N65535], (unsigned long long)n65535);
	__syncthreads();
	if (tid == 0) {
		unsigned long long ngood, c;
		if (shift == 8) {
			ngood = L.scal[SGQ_S_N65535];
			for (int b = 0; b < SGQ_HIST; b++)
				ngood += L.hist[b];
			L.scal[SGQ_S_NGOOD] = ngood;
			c = 0;
		} else {
			ngood = L.scal[SGQ_S_NGOOD];
			c = L.scal[SGQ_S_BEFORE];
		}
		unsigned long long bin = SGQ_HIST;
		for (int b = 0; b < SGQ_HIST; b++) {
			const unsigned long long nc = c + L.hist[b];
			if (2 * nc > ngood) {
				bin = (unsigned long long)b;
				break;
			}
			c = nc;
		}
		L.scal[SGQ_S_BIN] = bin;
		L.scal[SGQ_S_BEFORE] = c;
	}
	__syncthreads();
}

/* steps 2 to 6 for frame f and the clamped area (ax, ay): every thread returns the same record */
template <int T>
__device__ static __forceinline__ void sgq_frame(const SgSeqpsfParams &p, int f, int ax, int ay, const SgqLds &L, int tid,
		sg_seqpsf_frame &o) {
	const int w = p.w, h = p.h, ne = w * h;
	const uint16_t *img = p.img + (int64_t)f * p.frame_pitch + (int64_t)(p.H - ay - h) * p.row_pitch + ax;
	for (int q = tid; q < ne; q += T) {
		const int i = q / w, j = q - i * w;
		L.box[q] = img[(int64_t)i * p.row_pitch + j];
	}
	__syncthreads();
	sq_frame_clear(o, SG_FIT_NOT_ENOUGH_PIXELS);
	o.area_x = ax;
	o.area_y = ay;
	/* the non-zero median: the upper byte, then the lower byte among its values */
	sgq_select_pass<T>(L, ne, tid, 8, 0u);
	o.ngood = (int64_t)L.scal[SGQ_S_NGOOD];
	const unsigned hi = (unsigned)L.scal[SGQ_S_BIN];
	o.bg = 0.;
	if (hi < SGQ_HIST) {	/* workgroup-uniform */
		sgq_select_pass<T>(L, ne, tid, 0, hi);
		o.bg = (double)(hi * 256u + (unsigned)L.scal[SGQ_S_BIN]);
	}
	/* removeHotPixels and the first maximum in row-major order: the key orders by value, then by the
	 * smaller index */
	unsigned long long key = 0;
	for (int q = tid; q < ne; q += T) {
		const int i = q / w, j = q - i * w;
		const unsigned long long k = ((unsigned long long)sq_median3x3(L.box, h, w, i, j) << 32) | (unsigned long long)(0xFFFFFFFFu - (unsigned)q);
		key = k > key ? k : key;
	}
#pragma unroll
	for (int s = 32; s >= 1; s >>= 1) {
		const unsigned long long u = __shfl_xor(key, s, 64);
		key = u > key ? u : key;
	}
	if (T > 64) {
		if ((tid & 63) == 0)
			L.wkey[tid >> 6] = key;
		__syncthreads();
		key = L.wkey[0];
		for (int wv = 1; wv < T / 64; wv++)
			key = L.wkey[wv] > key ? L.wkey[wv] : key;
		__syncthreads();
	}
	const int best = (int)(0xFFFFFFFFu - (unsigned)(key & 0xFFFFFFFFull));
	sgp_init_walks(L.box, h, w, o.bg, best / w, best % w, (uint16_t)(key >> 32), o.init);
	SgqEval<T> ev = {L.box, L.part, w, ne, tid};
	sq_fit(ev, w, h, p.fit_angle, p.norm, p.scale_x, p.scale_y, o);
}

__device__ static inline void sgq_mark(sg_seqpsf_frame *rec, int status) {
	sg_seqpsf_frame o;
	sq_frame_clear(o, status);
	*rec = o;
}

/* ORIGINAL / REGISTERED: one workgroup per frame */
__global__ void __launch_bounds__(SGQ_THREADS) k_seqpsf_frames(SgSeqpsfParams p) {
	extern __shared__ __attribute__((aligned(16))) unsigned char s_mem[];
	const int f = blockIdx.x, tid = threadIdx.x;
	const SgSeqpsfItem it = p.items[f];
	if (!it.run) {	/* workgroup-uniform */
		if (tid == 0)
			sgq_mark(&p.rec[f], SG_SEQPSF_EXCLUDED);
		return;
	}
	const SgqLds L = sgq_lds(s_mem, p.lds_box, SGQ_THREADS / 64);
	int ax = it.x, ay = it.y;
	sq_enforce_area(p.W, p.H, p.w, p.h, &ax, &ay);	/* the plan's values already are inside */
	sg_seqpsf_frame o;
	sgq_frame<SGQ_THREADS>(p, f, ax, ay, L, tid, o);
	if (tid == 0)
		p.rec[f] = o;
}

/* FOLLOW_STAR: one workgroup walks the chain */
__global__ void __launch_bounds__(SGQ_THREADS) k_seqpsf_chain(SgSeqpsfParams p) {
	extern __shared__ __attribute__((aligned(16))) unsigned char s_mem[];
	const int tid = threadIdx.x;
	const SgqLds L = sgq_lds(s_mem, p.lds_box, SGQ_THREADS / 64);
	if (tid == 0) {
		L.scal[SGQ_S_AX] = (unsigned long long)(long long)p.start_x;
		L.scal[SGQ_S_AY] = (unsigned long long)(long long)p.start_y;
		L.scal[SGQ_S_STOP] = 0;
	}
	__syncthreads();
	for (int f = 0; f < p.nframes; f++) {
		const int run = p.items[f].run;
		const int stopped = (int)L.scal[SGQ_S_STOP];
		if (!run || stopped) {	/* workgroup-uniform; the chain passes over an excluded frame unchanged */
			if (tid == 0)
				sgq_mark(&p.rec[f], run ? SG_SEQPSF_NOT_RUN : SG_SEQPSF_EXCLUDED);
			continue;
		}
		int ax = (int)(long long)L.scal[SGQ_S_AX], ay = (int)(long long)L.scal[SGQ_S_AY];
		sq_enforce_area(p.W, p.H, p.w, p.h, &ax, &ay);
		sg_seqpsf_frame o;
		sgq_frame<SGQ_THREADS>(p, f, ax, ay, L, tid, o);
		if (tid == 0) {
			p.rec[f] = o;
			if (o.status == SG_FIT_STAR) {
				int nx, ny;
				sq_follow_area(o.xpos, o.ypos, p.w, p.h, &nx, &ny);
				L.scal[SGQ_S_AX] = (unsigned long long)(long long)nx;
				L.scal[SGQ_S_AY] = (unsigned long long)(long long)ny;
			} else {
				L.scal[SGQ_S_STOP] = 1;
			}
		}
		__syncthreads();	/* the carry is written, and the box is free for the next frame */
	}
	if (tid == 0) {
		p.carry[0] = (int)(long long)L.scal[SGQ_S_AX];
		p.carry[1] = (int)(long long)L.scal[SGQ_S_AY];
	}
}

/* one planned call on resident frames; *carry receives the carried area; ms / launches are added */
static int sgq_run(sg_ctx *ctx, int dev_index, const SgSeqpsfPlan &pl, const uint16_t *d_frames, sg_seqpsf_frame *per_frame,
		sg_rect *carry, void *stream, double *ms_sum, int *launches) {
	SgDevice &dv = ctx->dev[dev_index];
	HIPCHK(hipSetDevice(dv.id));
	hipStream_t s = sg_stream(dv, stream);
	HIPCHK(ensure(dv.seqpsf_work, pl.work_bytes));
	char *wk = (char *)dv.seqpsf_work.p;
	SgSeqpsfParams q;
	q.img = d_frames;
	q.frame_pitch = pl.frame_pitch;
	q.row_pitch = pl.row_pitch;
	q.W = pl.W;
	q.H = pl.H;
	q.w = pl.w;
	q.h = pl.h;
	q.nframes = pl.nframes;
	q.fit_angle = pl.fit_angle;
	q.lds_box = (unsigned)pl.lds_box;
	q.norm = pl.norm;
	q.scale_x = pl.scale_x;
	q.scale_y = pl.scale_y;
	q.items = (const SgSeqpsfItem *)wk;
	q.rec = (sg_seqpsf_frame *)(wk + pl.table_bytes);
	q.carry = (int *)(wk + pl.table_bytes + pl.record_bytes - 16);
	q.start_x = pl.start_x;
	q.start_y = pl.start_y;
	const bool chain = pl.framing == SG_SEQPSF_FOLLOW_STAR;
	int hcarry[2] = {pl.start_x, pl.start_y};
	HIPCHK(hipMemcpyAsync(wk, pl.items.data(), (size_t)pl.nframes * sizeof(SgSeqpsfItem), hipMemcpyHostToDevice, s));
	HIPCHK(hipEventRecord(dv.ev[0], s));
	if (chain)
		hipLaunchKernelGGL(k_seqpsf_chain, dim3(1), dim3(SGQ_THREADS), pl.lds_bytes, s, q);
	else
		hipLaunchKernelGGL(k_seqpsf_frames, dim3(pl.grid), dim3(SGQ_THREADS), pl.lds_bytes, s, q);
	HIPCHK(hipGetLastError());
	HIPCHK(hipEventRecord(dv.ev[1], s));
	HIPCHK(hipMemcpyAsync(per_frame, q.rec, (size_t)pl.nframes * sizeof(sg_seqpsf_frame), hipMemcpyDeviceToHost, s));
	if (chain)
		HIPCHK(hipMemcpyAsync(hcarry, q.carry, sizeof hcarry, hipMemcpyDeviceToHost, s));
	HIPCHK(hipStreamSynchronize(s));
	float ms = 0.f;
	HIPCHK(hipEventElapsedTime(&ms, dv.ev[0], dv.ev[1]));
	*ms_sum += ms;
	*launches += 1;
	carry->x = hcarry[0];
	carry->y = hcarry[1];
	carry->w = pl.w;
	carry->h = pl.h;
	return SG_OK;
}

static int sgq_check(sg_ctx *ctx, SgSeqpsfPlan &pl, const sg_seqpsf_desc *desc, const void *frames, int64_t frame_pitch,
		int64_t row_pitch, int W, int H, int nframes, const int *included, const int *reg_shiftx, const int *reg_shifty,
		const sg_seqpsf_frame *per_frame, const sg_rect *carry) {
	const int rc = sg_seqpsf_plan(desc, W, H, nframes, frame_pitch, row_pitch, included, reg_shiftx, reg_shifty, carry, pl);
	if (rc != SG_OK)
		return set_err(ctx, rc, "%s", pl.err);
	if (!frames || !per_frame)
		return set_err(ctx, SG_ERR_GENERIC, "seqpsf: missing frames or records%s", "");
	return SG_OK;
}

extern "C" int sg_seqpsf_u16_device(sg_ctx *ctx, int dev_index, const sg_seqpsf_desc *desc, const uint16_t *d_frames,
		int64_t frame_pitch, int64_t row_pitch, int W, int H, int nframes, const int *included, const int *reg_shiftx,
		const int *reg_shifty, sg_seqpsf_frame *per_frame, sg_rect *area_carry, void *stream) {
	if (!sg_dev_ok(ctx, dev_index))
		return SG_ERR_GENERIC;
	SgSeqpsfPlan pl;
	int rc = sgq_check(ctx, pl, desc, d_frames, frame_pitch, row_pitch, W, H, nframes, included, reg_shiftx, reg_shifty,
			per_frame, area_carry);
	if (rc != SG_OK)
		return rc;
	SgDevice &dv = ctx->dev[dev_index];
	sg_rect carry;
	double ms = 0.;
	int launches = 0;
	rc = sgq_run(ctx, dev_index, pl, d_frames, per_frame, &carry, stream, &ms, &launches);
	dv.seqpsf_ms = ms;
	dv.seqpsf_launches = launches;
	if (rc == SG_OK && area_carry)
		*area_carry = carry;
	return rc;
}

/* host frames: each batch's layers are uploaded tight and run as a sequence of their own; a
 * FOLLOW_STAR chain enters each batch with the area the last one left, and once it has stopped the
 * later batches are marked here without an upload */
extern "C" int sg_seqpsf_u16(sg_ctx *ctx, const sg_seqpsf_desc *desc, const uint16_t *frames, int64_t frame_pitch,
		int64_t row_pitch, int W, int H, int nframes, const int *included, const int *reg_shiftx, const int *reg_shifty,
		sg_seqpsf_frame *per_frame, sg_rect *area_carry) {
	if (!ctx || ctx->dev.empty())
		return SG_ERR_GENERIC;
	SgSeqpsfPlan pl;
	int rc = sgq_check(ctx, pl, desc, frames, frame_pitch, row_pitch, W, H, nframes, included, reg_shiftx, reg_shifty,
			per_frame, area_carry);
	if (rc != SG_OK)
		return rc;
	const size_t npix = (size_t)W * H;
	const bool chain = pl.framing == SG_SEQPSF_FOLLOW_STAR;
	SgHostBatches hb(ctx);
	HIPCHK(hb.begin(nframes, npix, SG_HOST_BUDGET_1G));
	sg_rect carry = {pl.start_x, pl.start_y, pl.w, pl.h};
	bool stopped = false;
	double ms = 0.;
	int launches = 0;
	while (hb.next()) {
		if (chain && stopped) {
			for (int f = 0; f < hb.nf; f++)
				sq_frame_clear(per_frame[hb.f0 + f], pl.items[(size_t)(hb.f0 + f)].run ? SG_SEQPSF_NOT_RUN : SG_SEQPSF_EXCLUDED);
			continue;
		}
		for (int f = 0; f < hb.nf; f++) {
			const int g = hb.f0 + f;
			if (pl.items[(size_t)g].run)
				HIPCHK(hb.upload_layer(hb.d + (size_t)f * npix, frames + (int64_t)g * pl.frame_pitch, W, H, pl.row_pitch));
		}
		SgSeqpsfPlan bp;
		rc = sg_seqpsf_plan(desc, W, H, hb.nf, 0, 0, included ? included + hb.f0 : nullptr, reg_shiftx ? reg_shiftx + hb.f0 : nullptr,
				reg_shifty ? reg_shifty + hb.f0 : nullptr, &carry, bp);
		if (rc != SG_OK)
			return set_err(ctx, rc, "%s", bp.err);
		rc = sgq_run(ctx, 0, bp, hb.d, per_frame + hb.f0, &carry, nullptr, &ms, &launches);
		if (rc != SG_OK)
			return rc;
		for (int f = 0; chain && f < hb.nf; f++) {
			const int st = per_frame[hb.f0 + f].status;
			stopped = stopped || (st != SG_FIT_STAR && st != SG_SEQPSF_EXCLUDED);
		}
	}
	hb.dv.seqpsf_ms = ms;
	hb.dv.seqpsf_launches = launches;
	if (area_carry)
		*area_carry = carry;
	return SG_OK;
}

extern "C" int sg_seqpsf_last_times(sg_ctx *ctx, int dev_index, double *ms, int *launches) {
	if (!sg_dev_ok(ctx, dev_index))
		return SG_ERR_GENERIC;
	const SgDevice &dv = ctx->dev[dev_index];
	if (ms)
		*ms = dv.seqpsf_ms;
	if (launches)
		*launches = dv.seqpsf_launches;
	return SG_OK;
}

extern "C" int sg_seqpsf_shifts(int nframes, int ref_image, const sg_seqpsf_frame *per_frame, int *shiftx, int *shifty,
		double *fwhm, int *best_index, double *best_fwhm) {
	if (nframes < 1 || !per_frame || !shiftx || !shifty)
		return -1;
	return sq_shifts(nframes, ref_image, per_frame, shiftx, shifty, fwhm, best_index, best_fwhm);
}
