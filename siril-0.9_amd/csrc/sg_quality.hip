/*
 * sg_quality.hip - QualityEstimate of whole resident layers (include/sirilgpu.h, sg_quality_u16*;
 * SURVEY.md §8f #9): the number register_ecc keeps per frame, for W x H planes read in place.  The
 * rule is sg_quality.h, the plan (checks, route, LDS layout, tiles, scratch, chunks) and the two
 * bookkeeping helpers sg_quality_plan.hpp.  The DFT path keeps its own kernels in sg_register.hip.
 *
 *   k_qest_resident  one workgroup per frame, no global scratch: the 3 x 3 samples go into LDS (two per
 *                    thread and step, by dword loads where the rows start on dwords), the
 *                    maximum is reduced there (wave shuffles, one LDS atomic per wave), the samples
 *                    are stretched in place, smoothed into a second LDS plane, and the gradient
 *                    runs over the margins' interior from that plane; the three integers become the
 *                    frame's double in the same workgroup.
 *   k_qest_sample    tiled route, pass 1: a 64 x 16 tile of samples to the u16 scratch plane, the
 *                    frame's maximum by one integer atomic per workgroup.
 *   k_qest_gradient  pass 2: the stretched tile with a halo of 2 (stretched on load) and the
 *                    smoothed tile with a halo of 1 in LDS, then the tile's terms; two integer
 *                    atomics per workgroup.  Tiles that lie outside the margins return at once.
 *   k_qest_finish    the frames' doubles.
 * Every sum is an integer, so the atomics' order does not matter: the same bits on every run.
 */
#include "sg_ctx.hpp"
#include "sg_quality_plan.hpp"
#include <algorithm>
#include <vector>

struct SgQualityAcc {
	uint32_t max, pad;
	unsigned long long val, pixels, pad2;
};
static_assert(sizeof(SgQualityAcc) == SGQ_ACC_BYTES, "accumulator layout");

struct SgQualityParams {
	const uint16_t *frames;
	int64_t fpitch, rpitch;
	sgq_geom g;
	const int *list;	/* the chunk's frames */
	double *out;		/* their results */
	uint16_t *planes;	/* tiled: the chunk's sample planes */
	SgQualityAcc *acc;	/* tiled: the chunk's accumulators */
	uint32_t plane_bytes;	/* P */
	int aligned;		/* sgq_rows_aligned: every row starts on a dword */
	int tiles_x;		/* tiled: blockIdx.x = ty * tiles_x + tx (a grid's y cannot hold a very tall plane's tiles) */
};

__device__ static inline uint32_t sgq_wave_max(uint32_t v) {
	for (int o = 32; o > 0; o >>= 1)
		v = max(v, (uint32_t)__shfl_xor((int)v, o));
	return v;
}

__device__ static inline unsigned long long sgq_wave_sum(unsigned long long v) {
	for (int o = 32; o > 0; o >>= 1)
		v += __shfl_xor(v, o);
	return v;
}

__global__ void __launch_bounds__(SGQ_RES_THREADS) k_qest_resident(SgQualityParams p) {
	extern __shared__ __align__(16) unsigned char q_lds[];
	uint16_t *smp = (uint16_t *)q_lds, *smo = (uint16_t *)(q_lds + p.plane_bytes);
	uint32_t *s_max = (uint32_t *)(q_lds + 2 * (size_t)p.plane_bytes);
	unsigned long long *s_acc = (unsigned long long *)(q_lds + 2 * (size_t)p.plane_bytes + 8);
	const int tid = threadIdx.x, xs = p.g.xs, ys = p.g.ys, ns = xs * ys;
	const uint16_t *img = p.frames + (int64_t)p.list[blockIdx.x] * p.fpitch;
	if (tid == 0) {
		*s_max = 0;
		s_acc[0] = s_acc[1] = 0;
	}
	__syncthreads();
	uint32_t mx = 0;
	const int hp = (xs + 1) / 2;	/* slots of two samples per row */
	for (int s = tid; s < hp * ys; s += SGQ_RES_THREADS) {
		const int y = s / hp, k = s - y * hp;
		uint32_t v[2];
		const int n = sgq_sample_slot(img, p.rpitch, p.aligned, xs, y, k, v);
		for (int j = 0; j < n; j++) {
			smp[y * xs + 2 * k + j] = (uint16_t)v[j];
			mx = max(mx, sgq_max_term(v[j], y, ys));
		}
	}
	mx = sgq_wave_max(mx);
	if ((tid & 63) == 0 && mx)
		atomicMax(s_max, mx);
	__syncthreads();
	const uint32_t m = *s_max;
	if (m) {
		const double mult = sgq_mult(m);
		for (int i = tid; i < ns; i += SGQ_RES_THREADS)
			smp[i] = (uint16_t)sgq_stretch(smp[i], m, mult);
		__syncthreads();
	}
	const sgq_view st = {smp, xs, 0, 0};
	for (int i = tid; i < ns; i += SGQ_RES_THREADS) {
		const int y = i / xs, x = i - y * xs;
		smo[i] = (uint16_t)sgq_smooth(st, x, y, xs, ys);
	}
	__syncthreads();
	const sgq_view sm = {smo, xs, 0, 0};
	const int iw = xs - 2 * p.g.xb, ih = ys - 2 * p.g.yb;
	unsigned long long val = 0, cnt = 0;
	if (iw > 0 && ih > 0)
		for (int i = tid; i < iw * ih; i += SGQ_RES_THREADS) {
			const int y = i / iw, x = i - y * iw;
			uint64_t t;
			if (sgq_gradient(sm, x + p.g.xb, y + p.g.yb, p.g, &t)) {
				val += t;
				cnt++;
			}
		}
	val = sgq_wave_sum(val);
	cnt = sgq_wave_sum(cnt);
	if ((tid & 63) == 0 && cnt) {
		atomicAdd(&s_acc[0], val);
		atomicAdd(&s_acc[1], cnt);
	}
	__syncthreads();
	if (tid == 0)
		p.out[blockIdx.x] = sgq_finish(s_acc[0], s_acc[1]);
}

__global__ void __launch_bounds__(SGQ_THREADS) k_qest_sample(SgQualityParams p) {
	__shared__ uint32_t s_max;
	const int tid = threadIdx.x, xs = p.g.xs, ys = p.g.ys;
	const int tx = blockIdx.x % p.tiles_x, ty = blockIdx.x / p.tiles_x;
	const uint16_t *img = p.frames + (int64_t)p.list[blockIdx.z] * p.fpitch;
	uint16_t *plane = p.planes + (size_t)blockIdx.z * (p.plane_bytes / sizeof(uint16_t));
	if (tid == 0)
		s_max = 0;
	__syncthreads();
	uint32_t mx = 0;
	for (int s = tid; s < SGQ_TILE_X / 2 * SGQ_TILE_Y; s += SGQ_THREADS) {	/* slots of two samples */
		const int ly = s / (SGQ_TILE_X / 2), k = tx * (SGQ_TILE_X / 2) + (s - ly * (SGQ_TILE_X / 2)), y = ty * SGQ_TILE_Y + ly;
		if (y >= ys || 2 * k >= xs)
			continue;
		uint32_t v[2];
		const int n = sgq_sample_slot(img, p.rpitch, p.aligned, xs, y, k, v);
		for (int j = 0; j < n; j++) {
			plane[(int64_t)y * xs + 2 * k + j] = (uint16_t)v[j];
			mx = max(mx, sgq_max_term(v[j], y, ys));
		}
	}
	mx = sgq_wave_max(mx);
	if ((tid & 63) == 0 && mx)
		atomicMax(&s_max, mx);
	__syncthreads();
	if (tid == 0 && s_max)
		atomicMax(&p.acc[blockIdx.z].max, s_max);
}

__global__ void __launch_bounds__(SGQ_THREADS) k_qest_gradient(SgQualityParams p) {
	__shared__ uint16_t s_st[SGQ_ST_W * SGQ_ST_H], s_sm[SGQ_SM_W * SGQ_SM_H];
	__shared__ unsigned long long s_acc[2];
	const int tid = threadIdx.x, xs = p.g.xs, ys = p.g.ys;
	const int tx0 = (int)(blockIdx.x % p.tiles_x) * SGQ_TILE_X, ty0 = (int)(blockIdx.x / p.tiles_x) * SGQ_TILE_Y;
	if (sgq_tile_idle(p.g, tx0, ty0))
		return;
	const uint16_t *plane = p.planes + (size_t)blockIdx.z * (p.plane_bytes / sizeof(uint16_t));
	const uint32_t m = p.acc[blockIdx.z].max;
	const double mult = m ? sgq_mult(m) : 0.0;
	if (tid == 0)
		s_acc[0] = s_acc[1] = 0;
	for (int i = tid; i < SGQ_ST_W * SGQ_ST_H; i += SGQ_THREADS)
		s_st[i] = sgq_tile_stretched(plane, xs, ys, tx0, ty0, i, m, mult);
	__syncthreads();
	for (int i = tid; i < SGQ_SM_W * SGQ_SM_H; i += SGQ_THREADS)
		s_sm[i] = sgq_tile_smoothed(s_st, xs, ys, tx0, ty0, i);
	__syncthreads();
	unsigned long long val = 0, cnt = 0;
	for (int i = tid; i < SGQ_TILE_X * SGQ_TILE_Y; i += SGQ_THREADS) {
		uint64_t t;
		if (sgq_tile_term(s_sm, p.g, tx0, ty0, i, &t)) {
			val += t;
			cnt++;
		}
	}
	val = sgq_wave_sum(val);
	cnt = sgq_wave_sum(cnt);
	if ((tid & 63) == 0 && cnt) {
		atomicAdd(&s_acc[0], val);
		atomicAdd(&s_acc[1], cnt);
	}
	__syncthreads();
	if (tid == 0 && s_acc[1]) {
		atomicAdd(&p.acc[blockIdx.z].val, s_acc[0]);
		atomicAdd(&p.acc[blockIdx.z].pixels, s_acc[1]);
	}
}

__global__ void __launch_bounds__(SGQ_THREADS) k_qest_finish(SgQualityParams p, int nf) {
	const int i = blockIdx.x * SGQ_THREADS + threadIdx.x;
	if (i < nf)
		p.out[i] = sgq_finish(p.acc[i].val, p.acc[i].pixels);
}

/* work: the frames to estimate, in index order; their results go to quality_raw[dest[k]] (dest == NULL: work[k]) */
static int sgq_run(sg_ctx *ctx, int dev_index, const SgQualityPlan &pl, const uint16_t *d_frames, const std::vector<int> &work,
		const int *dest, double *quality_raw, void *stream) {
	if (!dest)
		dest = work.data();
	SgDevice &dv = ctx->dev[dev_index];
	dv.quality_ms = 0.;
	dv.quality_route = pl.route;
	dv.quality_launches = 0;
	if (pl.route == SGQ_ROUTE_NONE) {
		for (size_t k = 0; k < work.size(); k++)
			quality_raw[dest[k]] = 0.0;
		return SG_OK;
	}
	if (work.empty())
		return SG_OK;
	HIPCHK(hipSetDevice(dv.id));
	hipStream_t s = sg_stream(dv, stream);
	HIPCHK(ensure(dv.quality_work, pl.total_bytes + 64));
	if (pl.route == SGQ_ROUTE_RESIDENT)
		HIPCHK(hipFuncSetAttribute((const void *)k_qest_resident, hipFuncAttributeMaxDynamicSharedMemorySize, SGQ_LDS_MAX));
	char *wk = (char *)dv.quality_work.p;
	const size_t o_list = 0, o_out = o_list + pl.list_bytes, o_acc = o_out + pl.out_bytes, o_planes = o_acc + pl.acc_bytes;
	SgQualityParams p;
	p.frames = d_frames;
	p.fpitch = pl.frame_pitch;
	p.rpitch = pl.row_pitch;
	p.g = pl.g;
	p.list = (const int *)(wk + o_list);
	p.out = (double *)(wk + o_out);
	p.acc = (SgQualityAcc *)(wk + o_acc);
	p.planes = (uint16_t *)(wk + o_planes);
	p.plane_bytes = (uint32_t)pl.plane_bytes;
	p.tiles_x = pl.tiles_x > 0 ? pl.tiles_x : 1;
	p.aligned = sgq_rows_aligned(d_frames, pl.frame_pitch, pl.row_pitch) ? 1 : 0;
	std::vector<double> hout((size_t)pl.chunk);
	for (size_t k0 = 0; k0 < work.size(); k0 += (size_t)pl.chunk) {
		const int nf = (int)std::min(work.size() - k0, (size_t)pl.chunk);
		HIPCHK(hipMemcpyAsync(wk + o_list, work.data() + k0, sizeof(int) * nf, hipMemcpyHostToDevice, s));
		HIPCHK(hipEventRecord(dv.ev[0], s));
		if (pl.route == SGQ_ROUTE_RESIDENT) {
			hipLaunchKernelGGL(k_qest_resident, dim3((unsigned)nf), dim3(SGQ_RES_THREADS), pl.lds_bytes, s, p);
			HIPCHK(hipGetLastError());
			dv.quality_launches += 1;
		} else {
			const dim3 grid((unsigned)pl.tiles_x * (unsigned)pl.tiles_y, 1, (unsigned)nf);
			HIPCHK(hipMemsetAsync(wk + o_acc, 0, (size_t)nf * SGQ_ACC_BYTES, s));
			hipLaunchKernelGGL(k_qest_sample, grid, dim3(SGQ_THREADS), 0, s, p);
			HIPCHK(hipGetLastError());
			hipLaunchKernelGGL(k_qest_gradient, grid, dim3(SGQ_THREADS), 0, s, p);
			HIPCHK(hipGetLastError());
			hipLaunchKernelGGL(k_qest_finish, dim3((unsigned)((nf + SGQ_THREADS - 1) / SGQ_THREADS)), dim3(SGQ_THREADS), 0, s, p, nf);
			HIPCHK(hipGetLastError());
			dv.quality_launches += 3;
		}
		HIPCHK(hipEventRecord(dv.ev[1], s));
		HIPCHK(hipMemcpyAsync(hout.data(), p.out, sizeof(double) * nf, hipMemcpyDeviceToHost, s));
		HIPCHK(hipStreamSynchronize(s));
		float ms = 0.f;
		HIPCHK(hipEventElapsedTime(&ms, dv.ev[0], dv.ev[1]));
		dv.quality_ms += ms;
		for (int k = 0; k < nf; k++)
			quality_raw[dest[k0 + k]] = hout[k];
	}
	return SG_OK;
}

static int sgq_check(sg_ctx *ctx, SgQualityPlan &pl, std::vector<int> &work, const void *frames, int64_t frame_pitch,
		int64_t row_pitch, int W, int H, int nframes, const int *included, const double *quality_raw) {
	/* the arguments first (nwork does not matter to them), then the frames to estimate */
	int rc = sg_quality_plan(W, H, nframes, -1, frame_pitch, row_pitch, 0, ctx->knobs.quality_route, ctx->knobs.quality_chunk,
			ctx->knobs.quality_lds, pl);
	if (rc != SG_OK)
		return set_err(ctx, rc, "%s", pl.err);
	if (!frames || !quality_raw)
		return set_err(ctx, SG_ERR_GENERIC, "quality: missing frames or result array%s", "");
	work.clear();
	for (int f = 0; f < nframes; f++)
		if (!included || included[f])
			work.push_back(f);
	rc = sg_quality_plan(W, H, nframes, (int)work.size(), frame_pitch, row_pitch, 0, ctx->knobs.quality_route,
			ctx->knobs.quality_chunk, ctx->knobs.quality_lds, pl);
	if (rc != SG_OK)
		return set_err(ctx, rc, "%s", pl.err);
	return SG_OK;
}

extern "C" int sg_quality_u16_device(sg_ctx *ctx, int dev_index, const uint16_t *d_frames, int64_t frame_pitch,
		int64_t row_pitch, int W, int H, int nframes, const int *included, double *quality_raw, void *stream) {
	if (!sg_dev_ok(ctx, dev_index))
		return SG_ERR_GENERIC;
	SgQualityPlan pl;
	std::vector<int> work;
	const int rc = sgq_check(ctx, pl, work, d_frames, frame_pitch, row_pitch, W, H, nframes, included, quality_raw);
	if (rc != SG_OK)
		return rc;
	return sgq_run(ctx, dev_index, pl, d_frames, work, nullptr, quality_raw, stream);
}

/* host frames: the included frames are uploaded tight in batches of at most 512 MiB and estimated as
 * a sequence of their own; a frame's result does not depend on its neighbours, so this equals the
 * device entry.  The timings of sg_quality_last_times are summed over the batches. */
extern "C" int sg_quality_u16(sg_ctx *ctx, const uint16_t *frames, int64_t frame_pitch, int64_t row_pitch, int W, int H,
		int nframes, const int *included, double *quality_raw) {
	if (!ctx || ctx->dev.empty())
		return SG_ERR_GENERIC;
	SgQualityPlan pl;
	std::vector<int> work;
	int rc = sgq_check(ctx, pl, work, frames, frame_pitch, row_pitch, W, H, nframes, included, quality_raw);
	if (rc != SG_OK)
		return rc;
	if (pl.route == SGQ_ROUTE_NONE || work.empty())
		return sgq_run(ctx, 0, pl, nullptr, work, nullptr, quality_raw, nullptr);
	const size_t npix = (size_t)W * H;
	SgHostBatches hb(ctx);
	HIPCHK(hb.begin((int)work.size(), npix, SG_HOST_BUDGET_512M, ctx->knobs.quality_chunk));
	std::vector<int> seq(hb.batch);
	double ms = 0.;
	int launches = 0;
	while (hb.next()) {
		const int k0 = hb.f0, nf = hb.nf;
		for (int k = 0; k < nf; k++) {
			seq[k] = k;
			HIPCHK(hb.upload_layer(hb.d + (size_t)k * npix, frames + (int64_t)work[k0 + k] * pl.frame_pitch, W, H, pl.row_pitch));
		}
		SgQualityPlan bp;
		rc = sg_quality_plan(W, H, nf, nf, 0, 0, 0, ctx->knobs.quality_route, ctx->knobs.quality_chunk, ctx->knobs.quality_lds, bp);
		if (rc != SG_OK)
			return set_err(ctx, rc, "%s", bp.err);
		rc = sgq_run(ctx, 0, bp, hb.d, std::vector<int>(seq.begin(), seq.begin() + nf), work.data() + k0, quality_raw, nullptr);
		if (rc != SG_OK)
			return rc;
		ms += hb.dv.quality_ms;
		launches += hb.dv.quality_launches;
	}
	hb.dv.quality_ms = ms;
	hb.dv.quality_launches = launches;
	return SG_OK;
}

extern "C" int sg_quality_last_times(sg_ctx *ctx, int dev_index, double *ms, int *route, int *launches) {
	if (!sg_dev_ok(ctx, dev_index))
		return SG_ERR_GENERIC;
	const SgDevice &dv = ctx->dev[dev_index];
	if (ms)
		*ms = dv.quality_ms;
	if (route)
		*route = dv.quality_route;
	if (launches)
		*launches = dv.quality_launches;
	return SG_OK;
}

extern "C" int sg_quality_normalize(int nframes, int ref_image, const double *quality_raw, const int *measured,
		const int *normalized, double *quality, double *q_min, double *q_max, int *q_index, char *msg, int msg_len) {
	return sgq_normalize(nframes, ref_image, quality_raw, measured, normalized, quality, q_min, q_max, q_index, msg, msg_len);
}

extern "C" int sg_quality_select(int nframes, const double *quality, const int *included, double percent, double *threshold,
		int *selected, int *nselected, char *msg, int msg_len) {
	return sgq_select(nframes, quality, included, percent, threshold, selected, nselected, msg, msg_len);
}
