/*
 * sg_cosme.hip - automatic cosmetic correction of resident frames (include/sirilgpu.h,
 * sg_cosme_autodetect*): autoDetect (src/algos/cosmetic_correction.c:384-435)
 * for every layer of every frame, in place in HBM.  The per-pixel rule is sg_cosme.h, the plan
 * sg_cosme_plan.hpp, the literal restatement tests/cosme_ref.py.
 *
 *   k_cosme_hist   a layer's 65536-bin histogram (u16 counter pairs in LDS per 65535-sample
 *                  workgroup, flushed with integer atomics, as k_findstar_hist).
 *   k_cosme_stat   from it ngood, the histogram median and the exact sum |v - bkg| over bins
 *                  1 .. 65535, so the frame is read once for its statistics; avgDev and the
 *                  layer's integer thresholds are finished in fp64 (sgc_rule_make).
 *   k_cosme_main   the scan against the ORIGINAL image: the u16 tile with a halo of 2 (plain) or
 *                  4 (CFA) in LDS; every pixel takes its own two integer tests, a hot candidate
 *                  its 3x3 sum.  The few that pass go to an LDS queue, are thinned by a 24-compare
 *                  counting bound on the median and only then sorted (sgc_median).  A hit leaves
 *                  its value in the sparse `state` plane and its kind bit; the frame itself is not
 *                  written.
 *   k_cosme_round  the scan-order dependence.  The serial result is the unique fixed point of
 *                  "decide every pixel from the corrected values of the earlier pixels of its
 *                  window and the original values of the later ones" (the system is triangular).
 *                  A pixel whose record changes puts the later pixels of its window that could ever
 *                  be corrected (sgc_own) on the next round's list, once each (a test-and-set bit
 *                  in the round's active plane); a round decides only the pixels of its list.  The
 *                  earliest listed pixel of a round reads final values only, so every round
 *                  finishes at least one pixel and chains resolve in as many rounds as they are
 *                  long, at a cost proportional to the chains.  Which thread wins a bit, and
 *                  whether a reader sees a neighbour's old or new record inside one round, changes
 *                  the order of the lists but not the fixed point: the result is the same bits on
 *                  every run.  A list that overflows its capacity is replaced by a walk over the
 *                  active plane, which always holds the whole set.
 *   k_cosme_commit walks the two kind planes, stores the corrected values into the frames and
 *                  counts ihot / icold per frame (integer atomics).
 */
#include "sg_ctx.hpp"
#include "sg_cosme_plan.hpp"
#include <algorithm>
#include <vector>

struct SgCosmeParams {
	uint16_t *frames;
	int64_t fstride, npix;
	int W, H, C, nf, halo;
	sgc_rule *rules;		/* [nf * C] */
	uint32_t *hist;			/* [nf * C][SGC_BINS] */
	uint16_t *state;		/* [chunk pixels] */
	uint32_t *hot, *cold, *act[2];	/* bit planes */
	uint32_t *list[2];
	uint32_t *cnt;			/* [SGC_NCOUNT] active counts of the group's rounds */
	unsigned long long *counts;	/* [nf][2]: icold, ihot */
	uint32_t list_cap;
	uint64_t plane_words;
	double sig0, sig1, amount;
	int is_cfa;
};

__global__ void __launch_bounds__(1024) k_cosme_hist(SgCosmeParams p) {
	extern __shared__ uint32_t lh[];	/* 32768 dwords: bin pairs */
	const int fl = blockIdx.y, f = fl / p.C, c = fl - f * p.C;
	const int64_t p0 = (int64_t)blockIdx.x * SGC_HIST_CHUNK;
	const int64_t p1 = p0 + SGC_HIST_CHUNK < p.npix ? p0 + SGC_HIST_CHUNK : p.npix;
	for (int i = threadIdx.x; i < SGC_BINS / 2; i += blockDim.x)
		lh[i] = 0;
	__syncthreads();
	const uint16_t *pl = p.frames + (int64_t)f * p.fstride + (int64_t)c * p.npix;
	for (int64_t q = p0 + threadIdx.x; q < p1; q += blockDim.x) {
		const uint32_t v = pl[q];
		atomicAdd(&lh[v >> 1], 1u << ((v & 1u) * 16u));
	}
	__syncthreads();
	uint32_t *h = p.hist + (size_t)fl * SGC_BINS;
	for (int i = threadIdx.x; i < SGC_BINS / 2; i += blockDim.x) {
		const uint32_t w = lh[i];
		if (w & 0xFFFFu)
			atomicAdd(&h[2 * i], w & 0xFFFFu);
		if (w >> 16)
			atomicAdd(&h[2 * i + 1], w >> 16);
	}
}

/* one workgroup per layer: thread t owns bins 64 t .. 64 t + 63 */
__global__ void __launch_bounds__(1024) k_cosme_stat(SgCosmeParams p) {
	__shared__ uint32_t part[1024];
	__shared__ unsigned long long acc;
	__shared__ uint32_t med;
	const int fl = blockIdx.x, t = threadIdx.x;
	const uint32_t *h = p.hist + (size_t)fl * SGC_BINS;
	if (t == 0) {
		acc = 0;
		med = 0;
	}
	uint32_t cm = 0;
	for (int b = t * 64; b < t * 64 + 64; b++)
		if (b >= 1 && b < SGC_BINS - 1)
			cm += h[b];
	part[t] = cm;
	__syncthreads();
	uint64_t before = 0, total = 0;
	for (int i = 0; i < 1024; i++) {
		const uint32_t c = part[i];
		before += i < t ? c : 0;
		total += c;
	}
	const uint64_t ngood = total + h[SGC_BINS - 1];
	uint64_t run = before;
	if (2 * run <= ngood && 2 * (run + cm) > ngood)	/* the crossing lies in this thread's bins */
		for (int b = t * 64; b < t * 64 + 64; b++) {
			if (b < 1 || b >= SGC_BINS - 1)
				continue;
			run += h[b];
			if (2 * run > ngood) {
				med = (uint32_t)b;
				break;
			}
		}
	__syncthreads();
	const int64_t bkg = (int64_t)med;
	uint64_t s = 0;
	for (int b = t * 64; b < t * 64 + 64; b++)
		if (b >= 1) {
			const int64_t d = (int64_t)b - bkg;
			s += (uint64_t)h[b] * (uint64_t)(d < 0 ? -d : d);
		}
	if (s)
		atomicAdd(&acc, (unsigned long long)s);
	__syncthreads();
	if (t == 0) {
		sgc_rule r;
		sgc_rule_make(&r, (int64_t)ngood, med, (uint64_t)acc, p.sig0, p.sig1, p.amount, p.is_cfa);
		p.rules[fl] = r;
	}
}

/* autoDetect fails the frame at its first layer without a non-zero pixel: that layer and the later
 * ones are not scanned */
__device__ __forceinline__ bool sgc_layer_runs(const SgCosmeParams &p, int f, int c) {
	for (int cc = 0; cc <= c; cc++)
		if (p.rules[f * p.C + cc].ngood <= 0)
			return false;
	return true;
}

/* put pixel `gid` on the list of the round that reads active plane / list `slot` and count
 * `cslot`, once */
__device__ __forceinline__ void sgc_activate(const SgCosmeParams &p, int slot, int cslot, uint32_t gid) {
	const uint32_t bit = 1u << (gid & 31u);
	const uint32_t old = atomicOr(&p.act[slot][gid >> 5], bit);
	if (old & bit)
		return;
	const uint32_t pos = atomicAdd(&p.cnt[cslot], 1u);
	if (pos < p.list_cap)
		p.list[slot][pos] = gid;
}

struct SgCosmeLds {
	uint16_t tile[SGC_MAX_IN_W * SGC_MAX_IN_H];
	uint16_t q1[SGC_TILE_W * SGC_TILE_H], q2[SGC_TILE_W * SGC_TILE_H];
	uint32_t n1, n2;
};

__global__ void __launch_bounds__(SGC_THREADS) k_cosme_main(SgCosmeParams p) {
	__shared__ SgCosmeLds L;
	const int fl = blockIdx.z, f = fl / p.C, c = fl - f * p.C, tid = threadIdx.x;
	if (!sgc_layer_runs(p, f, c))
		return;
	const sgc_rule r = p.rules[fl];
	if (r.hot_min > 65535 && r.cold_max < 0)
		return;		/* no pixel can be corrected */
	const int x0 = blockIdx.x * SGC_TILE_W, y0 = blockIdx.y * SGC_TILE_H;
	const int in_w = SGC_TILE_W + 2 * p.halo, in_h = SGC_TILE_H + 2 * p.halo;
	const uint16_t *plane = p.frames + (int64_t)f * p.fstride + (int64_t)c * p.npix;
	if (tid == 0)
		L.n1 = L.n2 = 0;
	for (int idx = tid; idx < in_w * in_h; idx += SGC_THREADS)
		L.tile[idx] = sgc_tile_load(idx, plane, p.W, p.H, x0, y0, p.halo);
	__syncthreads();
	SgcTileGet g;
	g.s = L.tile;
	g.x0 = x0;
	g.y0 = y0;
	g.halo = p.halo;
	g.in_w = in_w;
	{	/* every pixel: its own tests, a hot candidate's 3x3 average */
		const int ox = tid % SGC_TILE_W, oy0 = (tid / SGC_TILE_W) * SGC_ROWS, x = x0 + ox;
		if (x < p.W)
			for (int u = 0; u < SGC_ROWS; u++) {
				const int y = y0 + oy0 + u;
				if (y >= p.H)
					break;
				const uint32_t pixel = g.at(x, y);
				const int own = sgc_own(r, pixel);
				const uint32_t e = (uint32_t)((oy0 + u) * SGC_TILE_W + ox);
				if (own == SGC_HOT) {
					if ((int32_t)sgc_average(g, p.W, p.H, x, y, r.step) <= r.a_max)
						L.q1[atomicAdd(&L.n1, 1u)] = (uint16_t)e;
				} else if (own == SGC_COLD) {
					L.q2[atomicAdd(&L.n2, 1u)] = (uint16_t)(e | 0x8000u);
				}
			}
	}
	__syncthreads();
	const uint32_t n1 = L.n1;
	for (uint32_t i = tid; i < n1; i += SGC_THREADS) {	/* the counting bound on the median */
		const uint32_t e = L.q1[i];
		const int x = x0 + (int)(e % SGC_TILE_W), y = y0 + (int)(e / SGC_TILE_W);
		if (sgc_hot_maybe(g, p.W, p.H, x, y, r, g.at(x, y)))
			L.q2[atomicAdd(&L.n2, 1u)] = (uint16_t)e;
	}
	__syncthreads();
	const uint32_t n2 = L.n2;
	const uint32_t base = (uint32_t)fl * (uint32_t)p.npix;
	for (uint32_t i = tid; i < n2; i += SGC_THREADS) {	/* the full rule */
		const uint32_t e = L.q2[i], loc = e & 0x7FFFu;
		const int x = x0 + (int)(loc % SGC_TILE_W), y = y0 + (int)(loc / SGC_TILE_W);
		const uint32_t pixel = g.at(x, y);
		uint16_t val = 0;
		const int kind = sgc_decide(g, p.W, p.H, x, y, r, pixel, (e & 0x8000u) ? SGC_COLD : SGC_HOT, &val);
		if (kind == SGC_NONE)
			continue;
		const uint32_t gid = base + (uint32_t)y * (uint32_t)p.W + (uint32_t)x;
		p.state[gid] = val;
		atomicOr(kind == SGC_HOT ? &p.hot[gid >> 5] : &p.cold[gid >> 5], 1u << (gid & 31u));
		if (val == pixel)
			continue;
		for (int k = 0; k < 12; k++) {
			int xx, yy;
			if (sgc_later(k, x, y, p.W, p.H, r.step, &xx, &yy) && sgc_own(r, g.at(xx, yy)) != SGC_NONE)
				sgc_activate(p, 0, 0, base + (uint32_t)yy * (uint32_t)p.W + (uint32_t)xx);
		}
	}
}

/* decide listed pixel gid again from the records as they stand; r = the round's index in its group */
__device__ __forceinline__ void sgc_reexamine(const SgCosmeParams &p, int r, uint32_t gid) {
	const uint32_t fl = gid / (uint32_t)p.npix, pix = gid - fl * (uint32_t)p.npix;
	const int f = (int)fl / p.C, c = (int)fl - f * p.C;
	const sgc_rule rule = p.rules[fl];
	const uint16_t *plane = p.frames + (int64_t)f * p.fstride + (int64_t)c * p.npix;
	const uint32_t pixel = plane[pix];
	const int own = sgc_own(rule, pixel);
	const int x = (int)(pix % (uint32_t)p.W), y = (int)(pix / (uint32_t)p.W);
	const uint32_t w = gid >> 5, bit = 1u << (gid & 31u);
	const int oldkind = (SGC_LOAD_BITS(&p.hot[w]) & bit) ? SGC_HOT : ((SGC_LOAD_BITS(&p.cold[w]) & bit) ? SGC_COLD : SGC_NONE);
	const uint32_t oldval = oldkind ? p.state[gid] : pixel;
	SgcStateGet g;
	g.plane = plane;
	g.state = p.state + (size_t)fl * (size_t)p.npix;
	g.hot = p.hot;
	g.cold = p.cold;
	g.base = (uint64_t)fl * (uint64_t)p.npix;
	g.p = pix;
	g.W = p.W;
	uint16_t val = 0;
	int kind = SGC_NONE;
	if (own == SGC_COLD || (own == SGC_HOT && sgc_hot_maybe(g, p.W, p.H, x, y, rule, pixel)))
		kind = sgc_decide(g, p.W, p.H, x, y, rule, pixel, own, &val);
	if (kind == SGC_NONE)
		val = (uint16_t)pixel;
	if (kind == oldkind && val == oldval)
		return;
	if (kind != SGC_NONE) {
		p.state[gid] = val;
		__threadfence();
	}
	if (oldkind != SGC_NONE && oldkind != kind)
		atomicAnd(oldkind == SGC_HOT ? &p.hot[w] : &p.cold[w], ~bit);
	if (kind != SGC_NONE && oldkind != kind)
		atomicOr(kind == SGC_HOT ? &p.hot[w] : &p.cold[w], bit);
	const int nslot = (r + 1) & 1;
	for (int k = 0; k < 12; k++) {
		int xx, yy;
		if (sgc_later(k, x, y, p.W, p.H, rule.step, &xx, &yy) &&
				sgc_own(rule, plane[(int64_t)yy * p.W + xx]) != SGC_NONE)
			sgc_activate(p, nslot, r + 1, (uint32_t)g.base + (uint32_t)yy * (uint32_t)p.W + (uint32_t)xx);
	}
}

__global__ void __launch_bounds__(256) k_cosme_round(SgCosmeParams p, int r) {
	const uint32_t n = p.cnt[r];
	if (n == 0)
		return;
	const int slot = r & 1;
	const uint64_t tid = (uint64_t)blockIdx.x * 256 + threadIdx.x, nthr = (uint64_t)gridDim.x * 256;
	if (n <= p.list_cap) {
		for (uint64_t i = tid; i < n; i += nthr) {
			const uint32_t gid = p.list[slot][i];
			atomicAnd(&p.act[slot][gid >> 5], ~(1u << (gid & 31u)));
			sgc_reexamine(p, r, gid);
		}
		return;
	}
	for (uint64_t w = tid; w < p.plane_words; w += nthr) {	/* the list overflowed: the plane holds the whole set */
		uint32_t m = p.act[slot][w];
		if (!m)
			continue;
		p.act[slot][w] = 0;
		while (m) {
			const int b = __ffs((int)m) - 1;
			m &= m - 1;
			sgc_reexamine(p, r, (uint32_t)(w * 32 + (uint64_t)b));
		}
	}
}

#define SGC_COMMIT_WORDS 16	/* kind-plane words per thread */

__global__ void __launch_bounds__(256) k_cosme_commit(SgCosmeParams p) {
	__shared__ unsigned int s_n[2];
	const int tid = threadIdx.x;
	if (tid < 2)
		s_n[tid] = 0;
	__syncthreads();
	const uint64_t w0 = (uint64_t)blockIdx.x * (256 * SGC_COMMIT_WORDS);
	const uint64_t fpix = (uint64_t)p.C * (uint64_t)p.npix;
	const uint64_t f0 = (w0 * 32) / fpix;	/* the block's first frame: its counts are summed in LDS */
	unsigned int mine[2] = {0, 0};
	for (int k = 0; k < SGC_COMMIT_WORDS; k++) {
		const uint64_t w = w0 + (uint64_t)k * 256 + tid;
		if (w >= p.plane_words)
			break;
		const uint32_t h = p.hot[w], cd = p.cold[w];
		uint32_t m = h | cd;
		while (m) {
			const int b = __ffs((int)m) - 1;
			m &= m - 1;
			const uint64_t gid = w * 32 + (uint64_t)b;
			const uint64_t fl = gid / (uint64_t)p.npix, pix = gid - fl * (uint64_t)p.npix;
			const uint64_t f = fl / (uint64_t)p.C, c = fl - f * (uint64_t)p.C;
			p.frames[(int64_t)f * p.fstride + (int64_t)c * p.npix + (int64_t)pix] = p.state[gid];
			const int hot = (h >> b) & 1u;
			if (f == f0)
				mine[hot]++;
			else
				atomicAdd(&p.counts[f * 2 + hot], 1ull);
		}
	}
	if (mine[0])
		atomicAdd(&s_n[0], mine[0]);
	if (mine[1])
		atomicAdd(&s_n[1], mine[1]);
	__syncthreads();
	if (tid < 2 && s_n[tid])
		atomicAdd(&p.counts[f0 * 2 + tid], (unsigned long long)s_n[tid]);
}

static int sgc_run(sg_ctx *ctx, int dev_index, const SgCosmePlan &pl, uint16_t *d_frames, void *stream,
		sg_cosme_frame *out) {
	SgDevice &dv = ctx->dev[dev_index];
	HIPCHK(hipSetDevice(dv.id));
	hipStream_t s = sg_stream(dv, stream);
	HIPCHK(ensure(dv.cosme_work, pl.total_bytes + 64));
	HIPCHK(hipFuncSetAttribute((const void *)k_cosme_hist, hipFuncAttributeMaxDynamicSharedMemorySize,
			SGC_BINS / 2 * sizeof(uint32_t)));
	char *wk = (char *)dv.cosme_work.p;
	/* cleared per chunk: the four bit planes, the histograms, the counters (contiguous) */
	const size_t o_planes = 0, o_hist = o_planes + 4 * pl.plane_bytes, o_count = o_hist + pl.hist_bytes;
	const size_t o_cnt = o_count + sg_up16((size_t)pl.chunk * 2 * sizeof(uint64_t));
	const size_t o_clear_end = o_count + pl.count_bytes;
	const size_t o_rules = o_clear_end, o_list = o_rules + pl.rule_bytes, o_state = o_list + 2 * pl.list_bytes;
	SgCosmeParams p;
	p.fstride = pl.frame_stride;
	p.npix = pl.npix;
	p.W = pl.W;
	p.H = pl.H;
	p.C = pl.C;
	p.halo = pl.halo;
	p.rules = (sgc_rule *)(wk + o_rules);
	p.hist = (uint32_t *)(wk + o_hist);
	p.state = (uint16_t *)(wk + o_state);
	p.hot = (uint32_t *)(wk + o_planes);
	p.cold = (uint32_t *)(wk + o_planes + pl.plane_bytes);
	p.act[0] = (uint32_t *)(wk + o_planes + 2 * pl.plane_bytes);
	p.act[1] = (uint32_t *)(wk + o_planes + 3 * pl.plane_bytes);
	p.list[0] = (uint32_t *)(wk + o_list);
	p.list[1] = (uint32_t *)(wk + o_list + pl.list_bytes);
	p.cnt = (uint32_t *)(wk + o_cnt);
	p.counts = (unsigned long long *)(wk + o_count);
	p.list_cap = pl.list_cap;
	p.sig0 = pl.sig0;
	p.sig1 = pl.sig1;
	p.amount = pl.amount;
	p.is_cfa = pl.is_cfa;
	std::vector<sgc_rule> hrules((size_t)pl.chunk * pl.C);
	std::vector<unsigned long long> hcounts((size_t)pl.chunk * 2);
	uint32_t hcnt[SGC_NCOUNT];
	dv.cosme_stat_ms = dv.cosme_main_ms = dv.cosme_resolve_ms = 0.;
	dv.cosme_rounds = 0;
	dv.cosme_reexamined = 0;
	for (int f0 = 0; f0 < pl.nframes; f0 += pl.chunk) {
		const int nf = std::min(pl.nframes - f0, pl.chunk);
		const uint64_t px = (uint64_t)nf * (uint64_t)pl.C * (uint64_t)pl.npix;
		p.frames = d_frames + (int64_t)f0 * pl.frame_stride;
		p.nf = nf;
		p.plane_words = (px + 31) / 32;
		const unsigned layers = (unsigned)(nf * pl.C);
		HIPCHK(hipEventRecord(dv.ev[0], s));
		HIPCHK(hipMemsetAsync(wk, 0, o_clear_end, s));
		hipLaunchKernelGGL(k_cosme_hist, dim3((unsigned)pl.hist_blocks, layers), dim3(1024),
				SGC_BINS / 2 * sizeof(uint32_t), s, p);
		HIPCHK(hipGetLastError());
		hipLaunchKernelGGL(k_cosme_stat, dim3(layers), dim3(1024), 0, s, p);
		HIPCHK(hipGetLastError());
		HIPCHK(hipEventRecord(dv.ev[1], s));
		hipLaunchKernelGGL(k_cosme_main, dim3((unsigned)pl.tiles_x, (unsigned)pl.tiles_y, layers), dim3(SGC_THREADS), 0, s, p);
		HIPCHK(hipGetLastError());
		HIPCHK(hipEventRecord(dv.ev[2], s));
		for (uint64_t groups = 0;; groups++) {
			if (groups > px / SGC_GROUP + 1)	/* every round finishes a pixel: cannot happen */
				return set_err(ctx, SG_ERR_GENERIC, "cosme: the rounds did not end%s", "");
			for (int r = 0; r < SGC_GROUP; r++) {
				hipLaunchKernelGGL(k_cosme_round, dim3(SGC_ROUND_BLOCKS), dim3(256), 0, s, p, r);
				HIPCHK(hipGetLastError());
			}
			HIPCHK(hipMemcpyAsync(hcnt, p.cnt, sizeof hcnt, hipMemcpyDeviceToHost, s));
			HIPCHK(hipStreamSynchronize(s));
			for (int r = 0; r < SGC_GROUP; r++)
				if (hcnt[r]) {
					dv.cosme_rounds++;
					dv.cosme_reexamined += hcnt[r];
				}
			if (hcnt[SGC_GROUP] == 0)
				break;
			/* the next group's first round reads count 0 and, SGC_GROUP being even, the same slot */
			HIPCHK(hipMemcpyAsync(p.cnt, p.cnt + SGC_GROUP, sizeof(uint32_t), hipMemcpyDeviceToDevice, s));
			HIPCHK(hipMemsetAsync(p.cnt + 1, 0, SGC_GROUP * sizeof(uint32_t), s));
		}
		const uint64_t cblocks = (p.plane_words + 256 * SGC_COMMIT_WORDS - 1) / (256 * SGC_COMMIT_WORDS);
		hipLaunchKernelGGL(k_cosme_commit, dim3((unsigned)cblocks), dim3(256), 0, s, p);
		HIPCHK(hipGetLastError());
		HIPCHK(hipEventRecord(dv.ev[3], s));
		HIPCHK(hipMemcpyAsync(hrules.data(), p.rules, sizeof(sgc_rule) * layers, hipMemcpyDeviceToHost, s));
		HIPCHK(hipMemcpyAsync(hcounts.data(), p.counts, sizeof(unsigned long long) * 2 * nf, hipMemcpyDeviceToHost, s));
		HIPCHK(hipStreamSynchronize(s));
		float ms0 = 0.f, ms1 = 0.f, ms2 = 0.f;
		HIPCHK(hipEventElapsedTime(&ms0, dv.ev[0], dv.ev[1]));
		HIPCHK(hipEventElapsedTime(&ms1, dv.ev[1], dv.ev[2]));
		HIPCHK(hipEventElapsedTime(&ms2, dv.ev[2], dv.ev[3]));
		dv.cosme_stat_ms += ms0;
		dv.cosme_main_ms += ms1;
		dv.cosme_resolve_ms += ms2;
		for (int f = 0; f < nf; f++) {
			sg_cosme_frame &o = out[f0 + f];
			memset(&o, 0, sizeof o);
			o.failed_layer = -1;
			o.icold = (int64_t)hcounts[2 * f];
			o.ihot = (int64_t)hcounts[2 * f + 1];
			for (int c = 0; c < pl.C; c++) {
				const sgc_rule &r = hrules[(size_t)f * pl.C + c];
				if (r.ngood <= 0) {
					o.status = 1;
					o.failed_layer = c;
					break;
				}
				o.bkg[c] = r.bkg;
				o.avg_dev[c] = r.avg_dev;
			}
		}
	}
	return SG_OK;
}

static int sgc_check(sg_ctx *ctx, SgCosmePlan &pl, const sg_cosme_desc *desc, const void *frames, int nframes,
		int64_t frame_stride, const sg_cosme_frame *out) {
	const int rc = sg_cosme_plan(desc, nframes, frame_stride, 0, ctx->knobs.cosme_chunk, ctx->knobs.cosme_list, pl);
	if (rc != SG_OK)
		return set_err(ctx, rc, "%s", pl.err);
	if (!frames || !out)
		return set_err(ctx, SG_ERR_GENERIC, "cosme: missing frames or result array%s", "");
	return SG_OK;
}

extern "C" int sg_cosme_autodetect_device(sg_ctx *ctx, int dev_index, const sg_cosme_desc *desc, uint16_t *d_frames,
		int nframes, int64_t frame_stride, void *stream, sg_cosme_frame *out) {
	if (!sg_dev_ok(ctx, dev_index))
		return SG_ERR_GENERIC;
	SgCosmePlan pl;
	const int rc = sgc_check(ctx, pl, desc, d_frames, nframes, frame_stride, out);
	if (rc != SG_OK)
		return rc;
	return sgc_run(ctx, dev_index, pl, d_frames, stream, out);
}

/* host frames [nframes][C][H][W]: uploaded, corrected and downloaded in batches of at most 512 MiB;
 * frames are independent, so this equals the device entry */
extern "C" int sg_cosme_autodetect(sg_ctx *ctx, const sg_cosme_desc *desc, uint16_t *frames, int nframes,
		sg_cosme_frame *out) {
	if (!ctx || ctx->dev.empty())
		return SG_ERR_GENERIC;
	SgCosmePlan pl;
	int rc = sgc_check(ctx, pl, desc, frames, nframes, 0, out);
	if (rc != SG_OK)
		return rc;
	const size_t fpix = (size_t)pl.npix * pl.C;
	SgHostBatches hb(ctx);
	HIPCHK(hb.begin(nframes, fpix, SG_HOST_BUDGET_512M, ctx->knobs.cosme_chunk));
	while (hb.next()) {
		HIPCHK(hb.upload(frames));
		SgCosmePlan bp;
		rc = sg_cosme_plan(desc, hb.nf, 0, 0, ctx->knobs.cosme_chunk, ctx->knobs.cosme_list, bp);
		if (rc != SG_OK)
			return set_err(ctx, rc, "%s", bp.err);
		rc = sgc_run(ctx, 0, bp, hb.d, nullptr, out + hb.f0);
		if (rc != SG_OK)
			return rc;
		HIPCHK(hipMemcpyAsync(frames + (size_t)hb.f0 * fpix, hb.d, hb.bytes(), hipMemcpyDeviceToHost, hb.dv.stream));
		HIPCHK(hipStreamSynchronize(hb.dv.stream));
	}
	return SG_OK;
}

extern "C" int sg_cosme_last_times(sg_ctx *ctx, int dev_index, double *stat_ms, double *main_ms, double *resolve_ms,
		int *rounds, int64_t *reexamined) {
	if (!sg_dev_ok(ctx, dev_index))
		return SG_ERR_GENERIC;
	const SgDevice &dv = ctx->dev[dev_index];
	if (stat_ms)
		*stat_ms = dv.cosme_stat_ms;
	if (main_ms)
		*main_ms = dv.cosme_main_ms;
	if (resolve_ms)
		*resolve_ms = dv.cosme_resolve_ms;
	if (rounds)
		*rounds = dv.cosme_rounds;
	if (reexamined)
		*reexamined = (int64_t)dv.cosme_reexamined;
	return SG_OK;
}
