/*
 * sg_prepro.hip - sequence preprocessing on resident frames: the loop body of
 * seqpreprocess (src/core/siril.c:1019-1169) in place in HBM.  The per-sequence decisions (level,
 * thresholds, deviant list, schedule, search bookkeeping) are the host-only plan
 * (sg_prepro_plan.hpp); here are the three kernels and the C ABI (include/sirilgpu.h).
 *
 *   - k_prepro_calibrate: preprocess() (:945-961) and the subtraction of the fitted dark
 *     (:977-980) fused into one in-place pass.  A thread holds the masters of 8 pixels in
 *     registers and loops over the frames of the batch: 2 B read + 2 B written per pixel and
 *     frame, the masters read once per batch.  128-bit accesses when the frame base and stride
 *     are 16-byte aligned, a scalar loop for the tail (or for everything otherwise).
 *   - k_prepro_noise: one wave per (row, evaluation) of FnNoise1_ushort (quantize.c:658-783) on
 *     max(raw - round_to_WORD(dark * k), 0), formed on the fly.  A difference belongs to each
 *     non-zero pixel that has a non-zero predecessor in its row: the predecessor comes from the
 *     lane's own pixels, from a lower lane (ballot + shuffle of the 256-pixel step) or, across
 *     steps, from a carried value, so nothing is compacted and no LDS is used at any width.
 *     n, sum and sum of squares are 64-bit integers (exact, so their order is free); the
 *     up-to-three clip passes re-scan the row and re-derive their nested masks from the
 *     earlier (mean, stdev) pairs.
 *   - k_prepro_cosmetic: cosmeticCorrection (cosmetic_correction.c:275-294): one lane walks one
 *     component of the schedule in list order in one frame; components and frames in parallel.
 * Every double expression is written as the reference writes it (no contraction, Makefile).
 */
#include "sg_common.hpp"
#include "sg_ctx.hpp"
#include "sg_prepro_plan.hpp"
#include <vector>

#define SGP_CHUNK_FRAMES 128	/* frames per batch: bounds the search's row-result block (2 x 128 x H doubles) */

struct SgCalParams {
	uint16_t *frames;
	int64_t fstride;	/* elements */
	int nf;
	int64_t total;		/* C*H*W */
	const uint16_t *off;	/* null: no offset */
	const uint16_t *dark;	/* null: no dark step; with `k`: the fit's dark, scaled per frame */
	const uint16_t *flat;	/* null: no flat; zeros already 1 */
	const double *k;	/* device [nf], dark optimization only */
	double level;		/* (double)(float)level */
	int vec;		/* frames 16-byte aligned: 128-bit body */
};

/* one pixel: darkOptimization's subtraction, then preprocess() */
__device__ __forceinline__ uint32_t sgp_cal_px(uint32_t v, uint32_t o, uint32_t dk, uint32_t fl, const SgCalParams &p,
		double k) {
	if (p.k) {	/* imoper(brut, round_to_WORD(dark' * k), SUB) */
		const uint32_t s = sgp_rtw((double)dk * k);
		v = v > s ? v - s : 0u;
	}
	if (p.off)
		v = v > o ? v - o : 0u;
	if (p.dark && !p.k)
		v = v > dk ? v - dk : 0u;
	if (p.flat)	/* fdiv: a divide, then a multiply by the float level */
		v = sgp_rtw(p.level * ((double)v / (double)fl));
	return v;
}

__device__ __forceinline__ uint32_t sgp_cal_pair(uint32_t v, uint32_t o, uint32_t dk, uint32_t fl, const SgCalParams &p,
		double k) {
	const uint32_t lo = sgp_cal_px(v & 0xFFFFu, o & 0xFFFFu, dk & 0xFFFFu, fl & 0xFFFFu, p, k);
	const uint32_t hi = sgp_cal_px(v >> 16, o >> 16, dk >> 16, fl >> 16, p, k);
	return lo | (hi << 16);
}

__global__ void __launch_bounds__(256) k_prepro_calibrate(SgCalParams p) {
	const int64_t tid = (int64_t)blockIdx.x * 256 + threadIdx.x, nthr = (int64_t)gridDim.x * 256;
	const int64_t nvec = p.vec ? p.total >> 3 : 0;
	for (int64_t i = tid; i < nvec; i += nthr) {
		uint4 o = make_uint4(0, 0, 0, 0), dk = o, fl = make_uint4(0x10001u, 0x10001u, 0x10001u, 0x10001u);
		if (p.off)
			o = ((const uint4 *)p.off)[i];
		if (p.dark)
			dk = ((const uint4 *)p.dark)[i];
		if (p.flat)
			fl = ((const uint4 *)p.flat)[i];
		for (int f = 0; f < p.nf; f++) {
			uint4 *q = (uint4 *)(p.frames + (int64_t)f * p.fstride) + i;
			const double k = p.k ? p.k[f] : 0.0;
			uint4 r = *q;
			r.x = sgp_cal_pair(r.x, o.x, dk.x, fl.x, p, k);
			r.y = sgp_cal_pair(r.y, o.y, dk.y, fl.y, p, k);
			r.z = sgp_cal_pair(r.z, o.z, dk.z, fl.z, p, k);
			r.w = sgp_cal_pair(r.w, o.w, dk.w, fl.w, p, k);
			*q = r;
		}
	}
	for (int64_t i = nvec * 8 + tid; i < p.total; i += nthr) {
		const uint32_t o = p.off ? p.off[i] : 0u, dk = p.dark ? p.dark[i] : 0u, fl = p.flat ? p.flat[i] : 1u;
		for (int f = 0; f < p.nf; f++) {
			uint16_t *q = p.frames + (int64_t)f * p.fstride + i;
			*q = (uint16_t)sgp_cal_px(*q, o, dk, fl, p, p.k ? p.k[f] : 0.0);
		}
	}
}

struct SgNoiseParams {
	const uint16_t *frames;
	int64_t fstride;
	const uint16_t *dark;	/* layer 0 of the master dark */
	int W, H, nev;
	const int *ef;		/* [nev] frame of the evaluation */
	const double *ek;	/* [nev] its k */
	double *sd;		/* [nev][H] the row's final stdev */
	int *flag;		/* [nev][H] 1: the row contributes */
};

#define SGP_PPL 4	/* consecutive pixels per lane and step of the noise scan: 256 pixels per wave step */

/* one scan of the row: count, sum and sum of squares of the differences that pass the first NP
 * clip conditions; every lane returns the wave's totals.  A lane takes SGP_PPL consecutive
 * pixels of each 256-pixel step (the next step's loads are issued before this one is worked):
 * inside the lane the predecessor is the previous non-zero pixel, for the lane's first it is the
 * last non-zero pixel of the nearest lower lane that has one (one ballot and one shuffle per
 * step), else the value carried from the earlier steps */
template <int NP>
__device__ __forceinline__ void sgp_noise_scan(const uint16_t *__restrict__ raw, const uint16_t *__restrict__ dark, int W,
		double k, int lane, const double *mean, const double *sd, long long &n, long long &s, long long &s2) {
	long long ls = 0, ls2 = 0;
	int cnt = 0;
	uint32_t carry = 0;	/* last non-zero pixel of the earlier steps (0: none yet) */
	uint32_t r[SGP_PPL], dk[SGP_PPL];
#pragma unroll
	for (int j = 0; j < SGP_PPL; j++) {
		const int x = lane * SGP_PPL + j;
		r[j] = x < W ? raw[x] : 0u;
		dk[j] = x < W ? dark[x] : 0u;
	}
	for (int64_t x0 = 0; x0 < W; x0 += 64 * SGP_PPL) {	/* 64-bit: W may be close to 2^31 */
		uint32_t nr[SGP_PPL], nd[SGP_PPL];
#pragma unroll
		for (int j = 0; j < SGP_PPL; j++) {
			const int64_t x = x0 + 64 * SGP_PPL + lane * SGP_PPL + j;
			nr[j] = x < W ? raw[x] : 0u;
			nd[j] = x < W ? dark[x] : 0u;
		}
		uint32_t pv[SGP_PPL], last = 0;
#pragma unroll
		for (int j = 0; j < SGP_PPL; j++) {	/* a pixel past the row end has r = 0, so pv = 0 */
			const uint32_t sub = sgp_rtw((double)dk[j] * k);
			pv[j] = r[j] > sub ? r[j] - sub : 0u;
			last = pv[j] ? pv[j] : last;
		}
		const unsigned long long nz = __ballot(last != 0);
		const unsigned long long below = nz & ((1ull << lane) - 1ull);
		uint32_t prev = (uint32_t)__shfl((int)last, below ? 63 - __clzll((long long)below) : 0, 64);
		if (!below)
			prev = carry;
#pragma unroll
		for (int j = 0; j < SGP_PPL; j++)
			if (pv[j]) {
				if (prev) {
					const int d = (int)prev - (int)pv[j];
					bool keep = true;
#pragma unroll
					for (int c = 0; c < NP; c++)
						keep = keep && fabs(d - mean[c]) < 5. * sd[c];
					if (keep) {
						cnt++;
						ls += d;
						ls2 += (long long)d * d;
					}
				}
				prev = pv[j];
			}
		if (nz)	/* wave-uniform */
			carry = (uint32_t)__shfl((int)last, 63 - __clzll((long long)nz), 64);
#pragma unroll
		for (int j = 0; j < SGP_PPL; j++) {
			r[j] = nr[j];
			dk[j] = nd[j];
		}
	}
	long long lc = cnt;
	for (int o = 32; o > 0; o >>= 1) {
		lc += __shfl_xor(lc, o, 64);
		ls += __shfl_xor(ls, o, 64);
		ls2 += __shfl_xor(ls2, o, 64);
	}
	n = lc;
	s = ls;
	s2 = ls2;
}

__global__ void __launch_bounds__(256) k_prepro_noise(SgNoiseParams p) {
	const int lane = threadIdx.x & 63;
	const int64_t row_id = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
	if (row_id >= (int64_t)p.nev * p.H)
		return;		/* wave-uniform */
	const int e = (int)(row_id / p.H), y = (int)(row_id % p.H);
	const double k = p.ek[e];
	const uint16_t *raw = p.frames + (int64_t)p.ef[e] * p.fstride + (int64_t)y * p.W;
	const uint16_t *dark = p.dark + (int64_t)y * p.W;
	double mean[3] = {0., 0., 0.}, sd[3] = {0., 0., 0.}, out = 0.;
	long long n, s, s2;
	int contributes = 0;
	sgp_noise_scan<0>(raw, dark, p.W, k, lane, mean, sd, n, s, s2);
	if (n >= 2) {
		contributes = 1;
		long long nvals = n;
		sgp_mean_sigma_sums(n, s, s2, &mean[0], &sd[0]);
		out = sd[0];
		if (sd[0] > 0.) {	/* up to NITER = 3 passes, each stops when it drops nothing */
			sgp_noise_scan<1>(raw, dark, p.W, k, lane, mean, sd, n, s, s2);
			if (n != nvals) {
				nvals = n;
				sgp_mean_sigma_sums(n, s, s2, &mean[1], &sd[1]);
				out = sd[1];
				sgp_noise_scan<2>(raw, dark, p.W, k, lane, mean, sd, n, s, s2);
				if (n != nvals) {
					nvals = n;
					sgp_mean_sigma_sums(n, s, s2, &mean[2], &sd[2]);
					out = sd[2];
					sgp_noise_scan<3>(raw, dark, p.W, k, lane, mean, sd, n, s, s2);
					if (n != nvals) {
						double m3;
						sgp_mean_sigma_sums(n, s, s2, &m3, &out);
					}
				}
			}
		}
	}
	if (lane == 0) {
		p.sd[row_id] = out;
		p.flag[row_id] = contributes;
	}
}

struct SgCosParams {
	uint16_t *frames;
	int64_t fstride;
	int nf, W, H, step;
	const uint32_t *items, *comp_start;
	uint32_t ncomp;
};

/* getAverage3x3 (:102-126) */
__device__ __forceinline__ uint32_t sgp_hot_px(const uint16_t *buf, int W, int H, int x, int y, int step) {
	uint32_t sum = 0;
	int n = 0;
#pragma unroll
	for (int dy = -1; dy <= 1; dy++)
#pragma unroll
		for (int dx = -1; dx <= 1; dx++) {
			if (dx == 0 && dy == 0)
				continue;
			const int xx = x + dx * step, yy = y + dy * step;
			if (yy >= 0 && yy < H && xx >= 0 && xx < W) {
				sum += buf[xx + (int64_t)yy * W];
				n++;
			}
		}
	return n ? sgp_rtw((double)sum / n) : 0u;
}

/* getMedian5x5 (:34-67): the median of {0} and the n - 1 smallest of the n in-frame neighbours
 * (sgp_correct_one), the two order statistics picked by rank counting over registers */
__device__ __forceinline__ uint32_t sgp_cold_px(const uint16_t *buf, int W, int H, int x, int y, int step) {
	uint32_t v[24];
	int n = 0;
#pragma unroll
	for (int i = 0; i < 25; i++) {
		if (i == 12)
			continue;
		const int xx = x + (i % 5 - 2) * step, yy = y + (i / 5 - 2) * step;
		const bool in = yy >= 0 && yy < H && xx >= 0 && xx < W;
		v[i < 12 ? i : i - 1] = in ? (uint32_t)buf[xx + (int64_t)yy * W] : 0x10000u;	/* outside: above every value */
		n += in;
	}
	if (n == 0)
		return 0u;
	const int r0 = (n - 1) / 2 - 1, r1 = n / 2 - 1;	/* ranks among the neighbours; -1: the zero */
	uint32_t m0 = 0, m1 = 0;
#pragma unroll
	for (int i = 0; i < 24; i++) {
		int rank = 0;
#pragma unroll
		for (int j = 0; j < 24; j++)
			rank += (v[j] < v[i] || (v[j] == v[i] && j < i)) ? 1 : 0;
		if (rank == r0)
			m0 = v[i];
		if (rank == r1)
			m1 = v[i];
	}
	return sgp_rtw((n & 1) ? (double)m0 : ((double)m0 + (double)m1) / 2.0);
}

__global__ void __launch_bounds__(64) k_prepro_cosmetic(SgCosParams p) {
	const int64_t t = (int64_t)blockIdx.x * 64 + threadIdx.x;
	if (t >= (int64_t)p.ncomp * p.nf)
		return;
	const uint32_t comp = (uint32_t)(t / p.nf);
	uint16_t *buf = p.frames + (t % p.nf) * p.fstride;
	const uint32_t end = p.comp_start[comp + 1];
	for (uint32_t it = p.comp_start[comp]; it < end; it++) {
		const uint32_t e = p.items[it], pix = e & ~SGP_COLD;
		const int x = (int)(pix % (uint32_t)p.W), y = (int)(pix / (uint32_t)p.W);
		buf[pix] = (uint16_t)((e & SGP_COLD) ? sgp_cold_px(buf, p.W, p.H, x, y, p.step)
				: sgp_hot_px(buf, p.W, p.H, x, y, p.step));
	}
}

struct sg_prepro {
	sg_ctx *ctx = nullptr;
	int dev_index = 0;
	SgPreproPlan plan;
	uint16_t *d_off = nullptr, *d_dark = nullptr, *d_flat = nullptr, *d_darkfit = nullptr;
	uint32_t *d_items = nullptr, *d_comp_start = nullptr;
	SgBuf work;
	void *pin = nullptr;	/* pinned: the row results of one batch of evaluations */
	size_t pin_size = 0;
};

extern "C" void sg_prepro_free(sg_prepro *pp) {
	if (!pp)
		return;
	if (pp->ctx && pp->dev_index < (int)pp->ctx->dev.size())
		(void)hipSetDevice(pp->ctx->dev[pp->dev_index].id);
	void *bufs[] = {pp->d_off, pp->d_dark, pp->d_flat, pp->d_darkfit, pp->d_items, pp->d_comp_start, pp->work.p};
	for (void *b : bufs)
		if (b)
			(void)hipFree(b);
	if (pp->pin)
		(void)hipHostFree(pp->pin);
	delete pp;
}

template <typename T> static hipError_t sgp_upload(T *&dst, const T *src, size_t n, hipStream_t s) {
	hipError_t e = hipMalloc((void **)&dst, n * sizeof(T) + 16);
	if (e == hipSuccess)
		e = hipMemcpyAsync(dst, src, n * sizeof(T), hipMemcpyHostToDevice, s);
	return e;
}

static int sgp_create(sg_ctx *ctx, sg_prepro *pp, const sg_prepro_desc *desc, hipStream_t s) {
	const SgPreproPlan &pl = pp->plan;
	const size_t npix = (size_t)pl.W * pl.H, total = npix * pl.C;
	if (pl.use_offset)
		HIPCHK(sgp_upload(pp->d_off, desc->offset, total, s));
	if (pl.use_dark)
		HIPCHK(sgp_upload(pp->d_dark, desc->dark, total, s));
	if (pl.use_flat)
		HIPCHK(sgp_upload(pp->d_flat, pl.flat1.data(), total, s));
	if (!pl.darkfit.empty())
		HIPCHK(sgp_upload(pp->d_darkfit, pl.darkfit.data(), npix, s));
	if (!pl.items.empty()) {
		HIPCHK(sgp_upload(pp->d_items, pl.items.data(), pl.items.size(), s));
		HIPCHK(sgp_upload(pp->d_comp_start, pl.comp_start.data(), pl.comp_start.size(), s));
	}
	HIPCHK(hipStreamSynchronize(s));
	return SG_OK;
}

extern "C" int sg_prepro_create(sg_ctx *ctx, int dev_index, const sg_prepro_desc *desc, sg_prepro **out) {
	if (!sg_dev_ok(ctx, dev_index) || !out)
		return SG_ERR_GENERIC;
	*out = nullptr;
	sg_prepro *pp = new sg_prepro;
	pp->ctx = ctx;
	pp->dev_index = dev_index;
	int rc = sg_prepro_plan(desc, pp->plan);
	if (rc != SG_OK) {
		rc = set_err(ctx, rc, "%s", pp->plan.err);
		delete pp;
		return rc;
	}
	SgDevice &dv = ctx->dev[dev_index];
	if (hipSetDevice(dv.id) != hipSuccess) {
		delete pp;
		return set_err(ctx, SG_ERR_DEVICE, "hipSetDevice failed%s", "");
	}
	rc = sgp_create(ctx, pp, desc, dv.stream);
	if (rc != SG_OK) {
		sg_prepro_free(pp);
		return rc;
	}
	*out = pp;
	return SG_OK;
}

extern "C" int sg_prepro_get_info(const sg_prepro *pp, sg_prepro_info *info) {
	if (!pp || !info)
		return SG_ERR_GENERIC;
	const SgPreproPlan &pl = pp->plan;
	info->level = (double)pl.level;
	info->icold = pl.icold;
	info->ihot = pl.ihot;
	info->thres_cold = pl.thres_cold;
	info->thres_hot = pl.thres_hot;
	info->dark_sigma = pl.dark_sigma;
	info->dark_median = pl.dark_median;
	info->cosmetic_applies = pl.cosme_applies;
	info->components = pl.comp_start.empty() ? 0 : (int64_t)pl.comp_start.size() - 1;
	info->longest_component = pl.longest;
	return SG_OK;
}

/* device block of one batch of evaluations: ek[cap] doubles, sd[cap * H] doubles, kfit[cap / 2]
 * doubles, then ef[cap] and flag[cap * H] ints */
struct SgpWork {
	double *ek, *sd, *kfit;
	int *ef, *flag;
};

static int sgp_work(sg_ctx *ctx, sg_prepro *pp, int cap, SgpWork &w) {
	const size_t H = (size_t)pp->plan.H;
	const size_t nd = (size_t)cap + (size_t)cap * H + (size_t)cap, ni = (size_t)cap + (size_t)cap * H;
	HIPCHK(ensure(pp->work, nd * sizeof(double) + ni * sizeof(int)));
	w.ek = (double *)pp->work.p;
	w.sd = w.ek + cap;
	w.kfit = w.sd + (size_t)cap * H;
	w.ef = (int *)(w.kfit + cap);
	w.flag = w.ef + cap;
	return SG_OK;
}

/* objective values of nev evaluations (frame ef[e] of the batch at `frames`, scale ek[e]) */
static int sgp_run_noise(sg_ctx *ctx, sg_prepro *pp, hipStream_t s, const uint16_t *frames, int64_t fstride,
		const SgpWork &w, const std::vector<int> &ef, const std::vector<double> &ek, std::vector<double> &noise) {
	const SgPreproPlan &pl = pp->plan;
	const int nev = (int)ef.size(), H = pl.H;
	noise.assign(nev, 0.0);
	if (nev == 0 || pl.W < 3)	/* rows must have at least 3 pixels */
		return SG_OK;
	HIPCHK(hipMemcpyAsync(w.ef, ef.data(), sizeof(int) * nev, hipMemcpyHostToDevice, s));
	HIPCHK(hipMemcpyAsync(w.ek, ek.data(), sizeof(double) * nev, hipMemcpyHostToDevice, s));
	SgNoiseParams p;
	p.frames = frames;
	p.fstride = fstride;
	p.dark = pp->d_dark;
	p.W = pl.W;
	p.H = H;
	p.nev = nev;
	p.ef = w.ef;
	p.ek = w.ek;
	p.sd = w.sd;
	p.flag = w.flag;
	const int64_t rows = (int64_t)nev * H;
	hipLaunchKernelGGL(k_prepro_noise, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, s, p);
	HIPCHK(hipGetLastError());
	const size_t need = (size_t)rows * (sizeof(double) + sizeof(int));
	if (pp->pin_size < need) {
		if (pp->pin)
			(void)hipHostFree(pp->pin);
		pp->pin = nullptr;
		pp->pin_size = 0;
		HIPCHK(hipHostMalloc(&pp->pin, need, hipHostMallocDefault));
		pp->pin_size = need;
	}
	double *sd = (double *)pp->pin;
	int *flag = (int *)(sd + rows);
	HIPCHK(hipMemcpyAsync(sd, w.sd, sizeof(double) * rows, hipMemcpyDeviceToHost, s));
	HIPCHK(hipMemcpyAsync(flag, w.flag, sizeof(int) * rows, hipMemcpyDeviceToHost, s));
	HIPCHK(hipStreamSynchronize(s));
	for (int e = 0; e < nev; e++)
		noise[e] = sgp_noise_finish(sd + (size_t)e * H, flag + (size_t)e * H, H, pl.W);
	return SG_OK;
}

static int sgp_check_call(sg_ctx *ctx, int dev_index, const sg_prepro *pp, const void *d_frames, int nframes) {
	if (!sg_dev_ok(ctx, dev_index) || !pp || !d_frames || nframes < 1)
		return SG_ERR_GENERIC;
	if (pp->ctx != ctx || pp->dev_index != dev_index)
		return set_err(ctx, SG_ERR_GENERIC, "the preprocessing object was created for another context or device%s", "");
	return SG_OK;
}

extern "C" int sg_prepro_noise_device(sg_ctx *ctx, int dev_index, sg_prepro *pp, const uint16_t *d_frames, int nframes,
		int64_t frame_stride, const double *k, double *noise, void *stream) {
	int rc = sgp_check_call(ctx, dev_index, pp, d_frames, nframes);
	if (rc != SG_OK)
		return rc;
	if (!k || !noise)
		return SG_ERR_GENERIC;
	if (!pp->d_dark)
		return set_err(ctx, SG_ERR_GENERIC, "the noise of a dark-subtracted frame needs a master dark%s", "");
	SgDevice &dv = ctx->dev[dev_index];
	HIPCHK(hipSetDevice(dv.id));
	hipStream_t s = sg_stream(dv, stream);
	const SgPreproPlan &pl = pp->plan;
	if (frame_stride == 0)
		frame_stride = (int64_t)pl.C * pl.H * pl.W;
	SgpWork w;
	for (int f0 = 0; f0 < nframes; f0 += 2 * SGP_CHUNK_FRAMES) {
		const int nf = std::min(nframes - f0, 2 * SGP_CHUNK_FRAMES);
		if ((rc = sgp_work(ctx, pp, 2 * SGP_CHUNK_FRAMES, w)) != SG_OK)
			return rc;
		std::vector<int> ef(nf);
		std::vector<double> ek(k + f0, k + f0 + nf), val;
		for (int f = 0; f < nf; f++)
			ef[f] = f;
		if ((rc = sgp_run_noise(ctx, pp, s, d_frames + (int64_t)f0 * frame_stride, frame_stride, w, ef, ek, val)) != SG_OK)
			return rc;
		std::copy(val.begin(), val.end(), noise + f0);
	}
	return SG_OK;
}

extern "C" int sg_prepro_frames_device(sg_ctx *ctx, int dev_index, sg_prepro *pp, uint16_t *d_frames, int nframes,
		int64_t frame_stride, double *dark_k, void *stream) {
	int rc = sgp_check_call(ctx, dev_index, pp, d_frames, nframes);
	if (rc != SG_OK)
		return rc;
	SgDevice &dv = ctx->dev[dev_index];
	HIPCHK(hipSetDevice(dv.id));
	hipStream_t s = sg_stream(dv, stream);
	const SgPreproPlan &pl = pp->plan;
	const int64_t total = (int64_t)pl.C * pl.H * pl.W;
	if (frame_stride == 0)
		frame_stride = total;
	SgpWork w = {};
	for (int f0 = 0; f0 < nframes; f0 += SGP_CHUNK_FRAMES) {
		const int nf = std::min(nframes - f0, SGP_CHUNK_FRAMES);
		uint16_t *fr = d_frames + (int64_t)f0 * frame_stride;
		if (pl.optd) {
			/* goldenSectionSearch, iteration t of every frame of the batch in one launch */
			if ((rc = sgp_work(ctx, pp, 2 * SGP_CHUNK_FRAMES, w)) != SG_OK)
				return rc;
			std::vector<SgGolden> g(nf);
			for (SgGolden &q : g)
				q.init(0.0, 2.0, 1E-3);
			std::vector<int> ef;
			std::vector<double> ek, val;
			for (;;) {
				ef.clear();
				ek.clear();
				for (int f = 0; f < nf; f++) {
					double kk[2];
					const int n = g[f].want(kk);
					for (int j = 0; j < n; j++) {
						ef.push_back(f);
						ek.push_back(kk[j]);
					}
				}
				if (ef.empty())
					break;
				if ((rc = sgp_run_noise(ctx, pp, s, fr, frame_stride, w, ef, ek, val)) != SG_OK)
					return rc;
				size_t at = 0;
				for (int f = 0; f < nf; f++) {
					double kk[2];
					const int n = g[f].want(kk);
					g[f].feed(val.data() + at);
					at += n;
				}
			}
			std::vector<double> kfit(nf);
			for (int f = 0; f < nf; f++)
				kfit[f] = g[f].result();
			HIPCHK(hipMemcpyAsync(w.kfit, kfit.data(), sizeof(double) * nf, hipMemcpyHostToDevice, s));
			HIPCHK(hipStreamSynchronize(s));	/* kfit is a local */
			if (dark_k)
				std::copy(kfit.begin(), kfit.end(), dark_k + f0);
		} else if (dark_k)
			std::fill(dark_k + f0, dark_k + f0 + nf, 1.0);
		if (pl.use_offset || pl.use_dark || pl.use_flat) {
			SgCalParams p;
			p.frames = fr;
			p.fstride = frame_stride;
			p.nf = nf;
			p.total = total;
			p.off = pp->d_off;
			p.dark = pl.optd && pp->d_darkfit ? pp->d_darkfit : pp->d_dark;
			p.flat = pp->d_flat;
			p.k = pl.optd ? w.kfit : nullptr;
			p.level = (double)pl.level;
			p.vec = ((uintptr_t)fr % 16 == 0 && frame_stride % 8 == 0) ? 1 : 0;
			const int64_t units = p.vec ? (total >> 3) + 8 : total;
			const unsigned blocks = (unsigned)std::min<int64_t>((units + 255) / 256, 4096);
			hipLaunchKernelGGL(k_prepro_calibrate, dim3(blocks), dim3(256), 0, s, p);
			HIPCHK(hipGetLastError());
		}
		if (pl.cosme_applies && !pl.items.empty()) {
			SgCosParams p;
			p.frames = fr;
			p.fstride = frame_stride;
			p.nf = nf;
			p.W = pl.W;
			p.H = pl.H;
			p.step = pl.is_cfa ? 2 : 1;
			p.items = pp->d_items;
			p.comp_start = pp->d_comp_start;
			p.ncomp = (uint32_t)(pl.comp_start.size() - 1);
			const int64_t threads = (int64_t)p.ncomp * nf;
			hipLaunchKernelGGL(k_prepro_cosmetic, dim3((unsigned)((threads + 63) / 64)), dim3(64), 0, s, p);
			HIPCHK(hipGetLastError());
		}
	}
	HIPCHK(hipStreamSynchronize(s));
	return SG_OK;
}

extern "C" int sg_prepro_frames(sg_ctx *ctx, sg_prepro *pp, uint16_t *frames, int nframes, double *dark_k) {
	int rc = sgp_check_call(ctx, 0, pp, frames, nframes);
	if (rc != SG_OK)
		return rc;
	const size_t total = (size_t)pp->plan.C * pp->plan.H * pp->plan.W;
	/* a batch is at most one chunk of the device entry */
	SgHostBatches hb(ctx);
	HIPCHK(hb.begin(nframes, total, SG_HOST_BUDGET_1G, SGP_CHUNK_FRAMES));
	while (hb.next()) {
		HIPCHK(hb.upload(frames));
		if ((rc = sg_prepro_frames_device(ctx, 0, pp, hb.d, hb.nf, 0, dark_k ? dark_k + hb.f0 : nullptr, nullptr)) != SG_OK)
			return rc;
		HIPCHK(hipMemcpyAsync(frames + (size_t)hb.f0 * total, hb.d, hb.bytes(), hipMemcpyDeviceToHost, hb.dv.stream));
		HIPCHK(hipStreamSynchronize(hb.dv.stream));
	}
	return SG_OK;
}
