/*
 * sg_findstar.hip - star candidates (include/sirilgpu.h, sg_findstar*): the whole-image part of
 * peaker (src/algos/star_finder.c:103-255) on frames resident in HBM.
 *   - k_findstar_hist: the chosen layer's 65536-bin histogram per frame, all values binned (u16
 *     counter pairs in LDS per 65535-sample chunk, as k_ikss_hist of sg_stats.hip does, flushed
 *     with global atomics); k_findstar_stat: from it the exact ngood, sum v, sum v^2 (u64) and the
 *     median of computeHisto / siril_stats_ushort_median.  The host finishes sigma and the
 *     threshold (sg_findstar_plan.hpp).
 *   - k_findstar_plane: plane 2 of the three-plane a-trous B3-spline transform, i.e. two
 *     pave_2d_bspline_smooth passes (Step 1, Step 2) fused per tile: the u16 tile with a halo of 6
 *     in LDS (loaded through the clamp, so pass 1 indexes it plainly), the pass-1 floats of the
 *     in-image positions with a halo of 4 in LDS, pass 2 from LDS with the clamp applied to its
 *     indices; rounded to WORD, a float maximum above 65535 kept (reget_rawdata's ratio).
 *   - k_findstar_peak: the 3x3 peak test, one wave per display row, a 64-bit mask per 64 columns
 *     and the row's count; k_findstar_scan: the exclusive scan of the row counts; k_findstar_emit:
 *     the candidates written at row offset + rank inside the row, which is the raster order of the
 *     reference's single-thread loop, the first `capacity` of them kept.
 *   - k_findstar_boxes: one wave per stored candidate gathers its 2r x 2r box of the original image.
 * Fitted stars (sg_findstar_fit*), the second half of peaker, on the candidate list k_findstar_emit
 * leaves on the device:
 *   - k_starfit_fit: one wave per stored candidate.  Its box goes into LDS as u16, pixels strided
 *     over the 64 lanes; each lane sums its share of J^T J, J^T f and |f|^2 in fp64 (one exp per
 *     pixel and evaluation), a butterfly of fixed order adds the lanes, so every lane holds the same
 *     bits and runs the 6 x 6 solver of sg_psf.h redundantly with uniform branches.  Lane 0 writes
 *     the candidate's record with its status (is_star included).
 *   - k_starfit_select: one wave per frame scans the statuses in candidate order, keeps the first
 *     max_stars accepted as compact sg_star records and marks the rest SG_FIT_OVER_CAP.
 *   The host downloads the stars (and the candidate records when asked) and sorts each frame's
 *   stars by (mag, cand).
 * The frames are only read.
 */
#include "sg_common.hpp"
#include "sg_ctx.hpp"
#include "sg_findstar_plan.hpp"
#include "sg_starfit_plan.hpp"
#include "sg_psf.h"
#include <algorithm>
#include <vector>

#define SGF_CHUNK 65535		/* samples per histogram workgroup: the u16 LDS counters cannot wrap */

/* histogram of plane `fr + f * fstride` into hist[f][v] */
__global__ void __launch_bounds__(1024)
k_findstar_hist(const uint16_t *__restrict__ fr, int64_t fstride, int64_t npix, uint32_t *__restrict__ hist) {
	extern __shared__ uint32_t lh[];	/* 32768 dwords: bin pairs */
	const int f = blockIdx.y;
	const int64_t p0 = (int64_t)blockIdx.x * SGF_CHUNK;
	const int64_t p1 = p0 + SGF_CHUNK < npix ? p0 + SGF_CHUNK : npix;
	for (int i = threadIdx.x; i < SGF_BINS / 2; i += blockDim.x)
		lh[i] = 0;
	__syncthreads();
	const uint16_t *pl = fr + (int64_t)f * fstride;
	for (int64_t p = p0 + threadIdx.x; p < p1; p += blockDim.x) {
		const uint32_t v = pl[p];
		atomicAdd(&lh[v >> 1], 1u << ((v & 1u) * 16u));
	}
	__syncthreads();
	uint32_t *h = hist + (size_t)f * SGF_BINS;
	for (int i = threadIdx.x; i < SGF_BINS / 2; i += blockDim.x) {
		const uint32_t w = lh[i];
		if (w & 0xFFFFu)
			atomicAdd(&h[2 * i], w & 0xFFFFu);
		if (w >> 16)
			atomicAdd(&h[2 * i + 1], w >> 16);
	}
}

/* stat[f] = {ngood, sum, sum2, median}: ngood the non-zero pixels; the median scans bins 1 .. 65534
 * (65535 is outside computeHisto's range) for the first running count above ngood / 2, else 0 */
__global__ void __launch_bounds__(1024) k_findstar_stat(const uint32_t *__restrict__ hist, uint64_t *__restrict__ stat) {
	__shared__ uint32_t part[1024];
	__shared__ unsigned long long acc[2];
	__shared__ uint32_t med;
	const int f = blockIdx.x, t = threadIdx.x;
	const uint32_t *h = hist + (size_t)f * SGF_BINS;
	if (t == 0) {
		acc[0] = acc[1] = 0;
		med = 0;
	}
	uint64_t s = 0, s2 = 0;
	uint32_t cm = 0;
	for (int b = t * 64; b < t * 64 + 64; b++) {
		const uint64_t c = h[b];
		s += c * (uint64_t)b;
		s2 += c * (uint64_t)b * (uint64_t)b;
		if (b >= 1 && b < SGF_BINS - 1)
			cm += (uint32_t)c;
	}
	part[t] = cm;
	__syncthreads();
	atomicAdd(&acc[0], (unsigned long long)s);
	atomicAdd(&acc[1], (unsigned long long)s2);
	/* every pixel is binned, so the bins sum to the plane: ngood = the bins above 0 */
	uint64_t before = 0, total = 0;
	for (int i = 0; i < 1024; i++) {
		const uint32_t c = part[i];
		before += i < t ? c : 0;
		total += c;
	}
	const uint64_t ngood = total + h[SGF_BINS - 1];
	uint64_t run = before;
	if (2 * run <= ngood && 2 * (run + cm) > ngood)	/* the crossing lies in this thread's bins */
		for (int b = t * 64; b < t * 64 + 64; b++) {
			if (b < 1 || b >= SGF_BINS - 1)
				continue;
			run += h[b];
			if (2 * run > ngood) {
				med = (uint32_t)b;
				break;
			}
		}
	__syncthreads();
	if (t == 0) {
		stat[4 * f] = ngood;
		stat[4 * f + 1] = acc[0];
		stat[4 * f + 2] = acc[1];
		stat[4 * f + 3] = med;
	}
}

struct SgPlaneParams {
	const uint16_t *in;	/* the layer of the first frame */
	int64_t fstride;
	uint16_t *out;		/* [nf][H][W] */
	uint32_t *fmax;		/* [nf] float bits of the plane's maximum where that exceeds 65535, else 0 */
	int W, H;
	double ratio;
};

/* one SGF_TILE_W x SGF_TILE_H tile of the detection plane of frame blockIdx.z */
static_assert(SGF_P2_ITEMS == 256 && SGF_MID_H % SGF_P1_ROWS == 0 && SGF_TILE_H % SGF_P2_ROWS == 0, "strips tile the block");
__global__ void __launch_bounds__(256) k_findstar_plane(SgPlaneParams p) {
	__shared__ uint16_t s_in[SGF_IN_H * SGF_IN_W];
	__shared__ float s_mid[SGF_MID_H * SGF_MID_W];
	const int f = blockIdx.z, tx0 = blockIdx.x * SGF_TILE_W, ty0 = blockIdx.y * SGF_TILE_H;
	const int W = p.W, H = p.H;
	const uint16_t *img = p.in + (int64_t)f * p.fstride;
	for (int idx = threadIdx.x; idx < SGF_IN_H * SGF_IN_W; idx += 256)
		s_in[idx] = sgf_tile_load(idx, img, W, H, tx0, ty0);
	__syncthreads();
	for (int item = threadIdx.x; item < SGF_P1_ITEMS; item += 256)
		sgf_tile_pass1(item, s_in, s_mid, W, H, tx0, ty0);
	__syncthreads();
	float mx = 0.f, v[SGF_P2_ROWS];
	int gy0, gx;
	const int n = sgf_tile_pass2(threadIdx.x, s_mid, W, H, tx0, ty0, &gy0, &gx, v);	/* SGF_P2_ITEMS == 256 */
#pragma unroll
	for (int u = 0; u < SGF_P2_ROWS; u++)
		if (u < n) {
			mx = fmaxf(mx, v[u]);
			p.out[((int64_t)f * H + gy0 + u) * W + gx] = sg_round_to_WORD((double)v[u] * p.ratio);
		}
	/* reget_rawdata needs the maximum only when it exceeds 65535 (no input reaches that: DESIGN.md);
	 * an atomic per wave on the frame's one word would serialise the whole grid */
	if (mx > 65535.f)
		atomicMax(&p.fmax[f], __float_as_uint(mx));
}

/* min(W, H) < 32: the detection plane is the image */
__global__ void __launch_bounds__(256) k_findstar_copy(const uint16_t *__restrict__ in, int64_t fstride, int64_t npix,
		uint16_t *__restrict__ out) {
	const int f = blockIdx.y;
	for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < npix; i += (int64_t)gridDim.x * 256)
		out[(int64_t)f * npix + i] = in[(int64_t)f * fstride + i];
}

struct SgPeakParams {
	const uint16_t *wave;	/* [nf][H][W], memory order */
	const uint16_t *img;	/* the layer of the first frame */
	int64_t fstride;
	int W, H, r, sx0, sy0, scan_w, scan_h, mask_words;
	const int *thr;			/* [nf]; 65535 lets nothing through */
	unsigned long long *mask;	/* [nf][scan_h][mask_words] */
	uint32_t *rows;			/* [nf][scan_h + 1]: counts, then exclusive offsets and the total */
	const unsigned long long *nst, *base;	/* [nf] stored candidates, first entry in xy / boxes */
	int *xy;
	uint16_t *boxes;
};

/* the peak test of display row sy0 + ry, one wave per row.  Display row y is memory row H - 1 - y,
 * so the row above (y - 1) is the next memory row.  r >= 1 and the area lies inside the image:
 * every neighbour is inside. */
__global__ void __launch_bounds__(256) k_findstar_peak(SgPeakParams p) {
	const int f = blockIdx.y, ry = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
	if (ry >= p.scan_h)
		return;
	const int W = p.W, y = p.sy0 + ry;
	const uint16_t *r0 = p.wave + ((int64_t)f * p.H + (p.H - 1 - y)) * W, *up = r0 + W, *dn = r0 - W;
	const int t = p.thr[f];
	unsigned long long *m = p.mask + ((size_t)f * p.scan_h + ry) * p.mask_words;
	uint32_t cnt = 0;
	for (int it = 0; it < p.mask_words; it++) {
		const int xo = it * 64 + lane, x = p.sx0 + xo;
		bool ok = false;
		if (xo < p.scan_w) {
			const int v = r0[x];
			if (v > t && v < 65535)
				ok = up[x - 1] < v && up[x] < v && up[x + 1] < v && r0[x - 1] < v && r0[x + 1] <= v &&
						dn[x - 1] <= v && dn[x] <= v && dn[x + 1] <= v;
		}
		const unsigned long long b = __ballot(ok);
		if (lane == 0)
			m[it] = b;
		cnt += (uint32_t)__popcll(b);
	}
	if (lane == 0)
		p.rows[(size_t)f * (p.scan_h + 1) + ry] = cnt;
}

/* rows[f][0 .. scan_h): counts -> exclusive offsets, rows[f][scan_h] = tot[f] = the frame's total */
__global__ void __launch_bounds__(64) k_findstar_scan(uint32_t *__restrict__ rows, int scan_h, uint32_t *__restrict__ tot) {
	uint32_t *r = rows + (size_t)blockIdx.x * (scan_h + 1);
	const int lane = threadIdx.x;
	uint32_t run = 0;
	for (int b0 = 0; b0 < scan_h; b0 += 64) {
		const int i = b0 + lane;
		const uint32_t c = i < scan_h ? r[i] : 0;
		uint32_t inc = c;
		for (int o = 1; o < 64; o <<= 1) {
			const uint32_t u = (uint32_t)__shfl_up((int)inc, o, 64);
			if (lane >= o)
				inc += u;
		}
		if (i < scan_h)
			r[i] = run + (inc - c);
		run += (uint32_t)__shfl((int)inc, 63, 64);
	}
	if (lane == 0) {
		r[scan_h] = run;
		tot[blockIdx.x] = run;
	}
}

/* candidate number (row offset + rank in the row) -> xy[base + number], below the capacity */
__global__ void __launch_bounds__(256) k_findstar_emit(SgPeakParams p) {
	const int f = blockIdx.y, ry = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
	if (ry >= p.scan_h)
		return;
	const uint32_t *rows = p.rows + (size_t)f * (p.scan_h + 1);
	unsigned long long off = rows[ry];
	const unsigned long long cap = p.nst[f], base = p.base[f];
	if (rows[ry + 1] == rows[ry] || off >= cap)
		return;
	const unsigned long long *m = p.mask + ((size_t)f * p.scan_h + ry) * p.mask_words;
	for (int it = 0; it < p.mask_words && off < cap; it++) {
		const unsigned long long b = m[it];
		if (!b)
			continue;
		const unsigned long long pos = off + (unsigned long long)__popcll(b & ((1ull << lane) - 1ull));
		if (((b >> lane) & 1ull) && pos < cap) {
			p.xy[2 * (base + pos)] = p.sx0 + it * 64 + lane;
			p.xy[2 * (base + pos) + 1] = p.sy0 + ry;
		}
		off += (unsigned long long)__popcll(b);
	}
}

/* boxes[g][ii * 2r + jj] = top[y - r + jj][x - r + ii] of the original image, one wave per stored
 * candidate; the scan rectangle keeps the box inside the area */
__global__ void __launch_bounds__(256) k_findstar_boxes(SgPeakParams p) {
	const int f = blockIdx.y, lane = threadIdx.x & 63;
	const unsigned long long ci = (unsigned long long)blockIdx.x * 4 + (threadIdx.x >> 6);
	if (ci >= p.nst[f])
		return;
	const unsigned long long g = p.base[f] + ci;
	const int x = p.xy[2 * g], y = p.xy[2 * g + 1], n2 = 2 * p.r;
	const uint16_t *img = p.img + (int64_t)f * p.fstride;
	uint16_t *box = p.boxes + (size_t)g * n2 * n2;
	for (int jj = 0; jj < n2; jj++) {
		const uint16_t *row = img + (int64_t)(p.H - 1 - (y - p.r + jj)) * p.W + (x - p.r);
		for (int ii = lane; ii < n2; ii += 64)
			box[(size_t)ii * n2 + jj] = row[ii];
	}
}

struct SgFitParams {
	const uint16_t *img;	/* the layer of the chunk's first frame */
	int64_t fstride;
	int W, H, r, max_stars;
	const unsigned long long *nst, *base;	/* [nf] stored candidates, first entry in xy / cands / stars */
	const int *xy;
	const double *bg;	/* [nf] the frame's median */
	double norm, scale_x, scale_y, roundness;
	sg_starfit_cand *cands;
	sg_star *stars;
	int *nstars;		/* [nf] */
};

/* the lanes' values added in a fixed order; every lane receives the same bits (IEEE addition
 * commutes, and each level adds the same two partial sums in both partner lanes) */
__device__ static inline double sgs_wave_sum(double v) {
#pragma unroll
	for (int o = 32; o >= 1; o >>= 1)
		v += __shfl_xor(v, o, 64);
	return v;
}

/* the evaluator of sgp_lm over a box in LDS: pixel p = i * n2 + j belongs to lane p % 64 */
struct SgPsfWaveEval {
	const uint16_t *box;
	int n2, ne, lane;
	template <int NP>
	__device__ void full(const double *x, SgPsfSums<NP> &s) const {
		sgp_sums_zero<NP>(s);
		const SgPsfModel<NP> m = sgp_model<NP>(x);
		for (int p = lane; p < ne; p += 64) {
			const int i = p / n2, j = p - i * n2;
			sgp_pixel<NP>(x, m, (double)(j + 1), (double)(i + 1), (double)box[p], s);
		}
#pragma unroll
		for (int k = 0; k < NP * (NP + 1) / 2; k++)
			s.a[k] = sgs_wave_sum(s.a[k]);
#pragma unroll
		for (int k = 0; k < NP; k++)
			s.g[k] = sgs_wave_sum(s.g[k]);
		s.ff = sgs_wave_sum(s.ff);
	}
	template <int NP>
	__device__ double resid(const double *x) const {
		const SgPsfModel<NP> m = sgp_model<NP>(x);
		double ff = 0.;
		for (int p = lane; p < ne; p += 64) {
			const int i = p / n2, j = p - i * n2;
			const double r = sgp_resid<NP>(x, m, (double)(j + 1), (double)(i + 1), (double)box[p]);
			ff += r * r;
		}
		return sgs_wave_sum(ff);
	}
	__device__ double flux(double B) const {
		double t = 0.;
		for (int p = lane; p < ne; p += 64)
			t += (double)box[p] - B;
		return sgs_wave_sum(t);
	}
};

/* waves per SIMD the fit kernel is compiled for (A/B: make EXTRA=-DSGS_OCC=n).  The solver's
 * dependent fp64 chains want a second wave to hide behind; a third or fourth costs more in
 * spills than it hides (profiles/starfit_64x4096.log). */
#ifndef SGS_OCC
#define SGS_OCC 2
#endif
#define SGS_OCC_ATTR __attribute__((amdgpu_waves_per_eu(SGS_OCC, SGS_OCC)))

/* one wave per stored candidate: box -> LDS, start values, fit, finish, is_star, record.  The scan
 * rectangle keeps the box inside the area, so every read is inside the image. */
__global__ void __launch_bounds__(64 * SGS_WAVES) SGS_OCC_ATTR k_starfit_fit(SgFitParams p) {
	extern __shared__ uint16_t s_box[];	/* SGS_WAVES boxes */
	const int f = blockIdx.y, wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
	const unsigned long long ci = (unsigned long long)blockIdx.x * SGS_WAVES + wv;
	const bool active = ci < p.nst[f];
	const int n2 = 2 * p.r, ne = n2 * n2;
	uint16_t *box = s_box + wv * ne;
	unsigned long long g = 0;
	int cx = 0, cy = 0;
	if (active) {
		g = p.base[f] + ci;
		cx = p.xy[2 * g];
		cy = p.xy[2 * g + 1];
		const uint16_t *img = p.img + (int64_t)f * p.fstride;
		for (int q = lane; q < ne; q += 64) {	/* box[ii * n2 + jj] = top[cy - r + jj][cx - r + ii] */
			const int ii = q / n2, jj = q - ii * n2;
			box[q] = img[(int64_t)(p.H - 1 - (cy - p.r + jj)) * p.W + (cx - p.r + ii)];
		}
	}
	__syncthreads();
	if (!active)
		return;
	/* removeHotPixels and the first maximum in row-major order: the key orders by value, then by
	 * the smaller index (ne <= 4096) */
	uint32_t key = 0;
	for (int q = lane; q < ne; q += 64) {
		const int i = q / n2, j = q - i * n2;
		const uint32_t k = ((uint32_t)sgp_median3x3(box, n2, i, j) << 16) | (uint32_t)(65535 - q);
		key = k > key ? k : key;
	}
#pragma unroll
	for (int o = 32; o >= 1; o >>= 1) {
		const uint32_t u = (uint32_t)__shfl_xor((int)key, o, 64);
		key = u > key ? u : key;
	}
	const int best = 65535 - (int)(key & 0xFFFFu);
	double init[SGP_NP];
	sgp_init_walks(box, n2, n2, p.bg[f], best / n2, best % n2, (uint16_t)(key >> 16), init);
	SgPsfWaveEval ev = {box, n2, ne, lane};
	SgPsfFit o;
	sgp_fit(ev, init, n2, cx, cy, p.norm, p.scale_x, p.scale_y, p.roundness, o);
	if (lane == 0) {
		sg_starfit_cand c;
		c.x = cx;
		c.y = cy;
		c.iters = o.iters;
		c.status = o.status;
		c.failed_test = o.failed_test;
		c.reserved = 0;
		for (int k = 0; k < SGP_NP; k++)
			c.init[k] = init[k];
		c.B = o.B;
		c.A = o.A;
		c.x0 = o.x0;
		c.y0 = o.y0;
		c.sx = o.sx;
		c.sy = o.sy;
		c.fwhmx = o.fwhmx;
		c.fwhmy = o.fwhmy;
		c.mag = o.mag;
		c.rmse = o.rmse;
		c.xpos = o.xpos;
		c.ypos = o.ypos;
		p.cands[g] = c;
	}
}

/* one wave per frame: the first max_stars accepted candidates in candidate order -> stars[base + rank],
 * the accepted ones beyond them marked SG_FIT_OVER_CAP, nstars[f] */
__global__ void __launch_bounds__(64) k_starfit_select(SgFitParams p) {
	const int f = blockIdx.x, lane = threadIdx.x;
	const unsigned long long n = p.nst[f], base = p.base[f];
	unsigned long long run = 0;
	for (unsigned long long c0 = 0; c0 < n; c0 += 64) {
		const unsigned long long c = c0 + lane;
		const bool acc = c < n && p.cands[base + c].status == SG_FIT_STAR;
		const unsigned long long b = __ballot(acc);
		const unsigned long long rank = run + (unsigned long long)__popcll(b & ((1ull << lane) - 1ull));
		if (acc) {
			sg_starfit_cand &q = p.cands[base + c];
			if (rank < (unsigned long long)p.max_stars) {
				sg_star st;
				st.cand = (int32_t)c;
				st.x = q.x;
				st.y = q.y;
				st.iters = q.iters;
				st.B = q.B;
				st.A = q.A;
				st.x0 = q.x0;
				st.y0 = q.y0;
				st.sx = q.sx;
				st.sy = q.sy;
				st.fwhmx = q.fwhmx;
				st.fwhmy = q.fwhmy;
				st.mag = q.mag;
				st.rmse = q.rmse;
				st.xpos = q.xpos;
				st.ypos = q.ypos;
				p.stars[base + rank] = st;
			} else
				q.status = SG_FIT_OVER_CAP;
		}
		run += (unsigned long long)__popcll(b);
	}
	if (lane == 0)
		p.nstars[f] = (int)(run < (unsigned long long)p.max_stars ? run : (unsigned long long)p.max_stars);
}

/* the body of sg_findstar_device; with a fit plan `fp` it goes on, chunk by chunk, to the fit of the
 * stored candidates (nstars, stars, cands of sg_findstar_fit_device; cand_xy and boxes are NULL) */
static int sgf_run(sg_ctx *ctx, int dev_index, const SgFindstarPlan &pl, const uint16_t *d_frames, int nframes,
		int64_t frame_stride, sg_findstar_frame *per_frame, int32_t *cand_xy, uint16_t *boxes, uint16_t *d_wave,
		void *stream, const SgStarfitPlan *fp, int32_t *nstars, sg_star *stars, sg_starfit_cand *cands) {
	SgDevice &dv = ctx->dev[dev_index];
	HIPCHK(hipSetDevice(dv.id));
	hipStream_t s = sg_stream(dv, stream);
	const int W = pl.W, H = pl.H;
	const int64_t npix = (int64_t)W * H;
	if (frame_stride == 0)
		frame_stride = npix * pl.C;
	const int chunk = sgf_chunk_frames(pl, nframes, d_wave != nullptr);
	/* the chunk's work block */
	const size_t o_hist = 0, o_stat = o_hist + sg_up16(pl.hist_bytes * chunk);
	const size_t o_fmax = o_stat + sg_up16(pl.stat_bytes * chunk), o_thr = o_fmax + sg_up16(sizeof(uint32_t) * chunk);
	const size_t o_nst = o_thr + sg_up16(sizeof(int) * chunk), o_rows = o_nst + sg_up16(2 * sizeof(uint64_t) * chunk);
	const size_t o_mask = o_rows + sg_up16(pl.rows_bytes * chunk), o_tot = o_mask + sg_up16(pl.mask_bytes * chunk);
	const size_t work_bytes = o_tot + sg_up16(sizeof(uint32_t) * chunk);
	HIPCHK(ensure(dv.fs_work, work_bytes));
	char *wk = (char *)dv.fs_work.p;
	uint32_t *hist = (uint32_t *)(wk + o_hist), *fmax = (uint32_t *)(wk + o_fmax), *rows = (uint32_t *)(wk + o_rows);
	uint32_t *tot = (uint32_t *)(wk + o_tot);
	uint64_t *stat = (uint64_t *)(wk + o_stat);
	int *thr = (int *)(wk + o_thr);
	unsigned long long *nst = (unsigned long long *)(wk + o_nst), *mask = (unsigned long long *)(wk + o_mask);
	if (!d_wave)
		HIPCHK(ensure(dv.fs_plane, pl.plane_bytes * chunk));
	(void)hipFuncSetAttribute((const void *)k_findstar_hist, hipFuncAttributeMaxDynamicSharedMemorySize,
			(int)(SGF_BINS / 2 * sizeof(uint32_t)));
	std::vector<uint64_t> hstat(4 * (size_t)chunk), hnst(2 * (size_t)chunk);
	std::vector<uint32_t> hfmax(chunk), htot(chunk);
	std::vector<int> hthr(chunk);
	std::vector<double> hmed(chunk);
	std::vector<uint16_t> hplane;
	if (fp)
		memset(nstars, 0, sizeof(int32_t) * nframes);
	for (int f0 = 0; f0 < nframes; f0 += chunk) {
		const int nf = std::min(nframes - f0, chunk);
		const uint16_t *lay = d_frames + (int64_t)f0 * frame_stride + (int64_t)pl.layer * npix;
		uint16_t *wave = d_wave ? d_wave + (int64_t)f0 * npix : (uint16_t *)dv.fs_plane.p;
		sg_findstar_frame *rec = per_frame + f0;
		/* statistics and the detection plane are independent: both queued before the first wait */
		HIPCHK(hipMemsetAsync(hist, 0, pl.hist_bytes * nf, s));
		HIPCHK(hipMemsetAsync(fmax, 0, sizeof(uint32_t) * nf, s));
		hipLaunchKernelGGL(k_findstar_hist, dim3((unsigned)((npix + SGF_CHUNK - 1) / SGF_CHUNK), (unsigned)nf), dim3(1024),
				SGF_BINS / 2 * sizeof(uint32_t), s, lay, frame_stride, npix, hist);
		HIPCHK(hipGetLastError());
		hipLaunchKernelGGL(k_findstar_stat, dim3((unsigned)nf), dim3(1024), 0, s, (const uint32_t *)hist, stat);
		HIPCHK(hipGetLastError());
		SgPlaneParams pp;
		pp.in = lay;
		pp.fstride = frame_stride;
		pp.out = wave;
		pp.fmax = fmax;
		pp.W = W;
		pp.H = H;
		pp.ratio = 1.0;
		if (pl.wavelet)
			hipLaunchKernelGGL(k_findstar_plane, dim3((unsigned)pl.tiles_x, (unsigned)pl.tiles_y, (unsigned)nf), dim3(256), 0,
					s, pp);
		else
			hipLaunchKernelGGL(k_findstar_copy, dim3((unsigned)std::min<int64_t>((npix + 255) / 256, 1024), (unsigned)nf),
					dim3(256), 0, s, lay, frame_stride, npix, wave);
		HIPCHK(hipGetLastError());
		HIPCHK(hipMemcpyAsync(hstat.data(), stat, pl.stat_bytes * nf, hipMemcpyDeviceToHost, s));
		HIPCHK(hipMemcpyAsync(hfmax.data(), fmax, sizeof(uint32_t) * nf, hipMemcpyDeviceToHost, s));
		HIPCHK(hipStreamSynchronize(s));
		for (int f = 0; f < nf; f++) {
			sg_findstar_frame &q = rec[f];
			memset(&q, 0, sizeof q);
			q.wavelet_applied = pl.wavelet;
			q.ngood = (int64_t)hstat[4 * f];
			hthr[f] = 65535;
			if (q.ngood == 0) {
				q.no_data = 1;
				continue;
			}
			q.median = (double)hstat[4 * f + 3];
			if (sgf_sums_exact(hstat[4 * f + 2]))
				q.sigma = sgf_sigma_sums(hstat[4 * f], hstat[4 * f + 1], hstat[4 * f + 2]);
			else {
				hplane.resize(npix);
				HIPCHK(hipMemcpyAsync(hplane.data(), lay + (int64_t)f * frame_stride, sizeof(uint16_t) * npix,
						hipMemcpyDeviceToHost, s));
				HIPCHK(hipStreamSynchronize(s));
				q.sigma = sgf_sigma_seq(hplane.data(), npix);
				q.sigma_on_host = 1;
			}
			q.threshold = sgf_threshold(q.median, q.sigma, pl.k, &q.threshold_wrapped);
			hthr[f] = q.threshold;
			/* reget_rawdata: a maximum above 65535 rescales that frame's plane */
			float mx;
			memcpy(&mx, &hfmax[f], sizeof mx);
			if (pl.wavelet && mx > 65535.f) {
				SgPlaneParams pr = pp;
				pr.in = lay + (int64_t)f * frame_stride;
				pr.out = wave + (int64_t)f * npix;
				pr.fmax = fmax + f;
				pr.ratio = 65535.0 / (double)mx;
				hipLaunchKernelGGL(k_findstar_plane, dim3((unsigned)pl.tiles_x, (unsigned)pl.tiles_y, 1u), dim3(256), 0, s, pr);
				HIPCHK(hipGetLastError());
				q.ratio_applied = 1;
			}
		}
		if (pl.scan_w == 0) {	/* 2r >= a side of the area: nothing to scan */
			HIPCHK(hipStreamSynchronize(s));
			continue;
		}
		SgPeakParams kp;
		kp.wave = wave;
		kp.img = lay;
		kp.fstride = frame_stride;
		kp.W = W;
		kp.H = H;
		kp.r = pl.r;
		kp.sx0 = pl.sx0;
		kp.sy0 = pl.sy0;
		kp.scan_w = pl.scan_w;
		kp.scan_h = pl.scan_h;
		kp.mask_words = pl.mask_words;
		kp.thr = thr;
		kp.mask = mask;
		kp.rows = rows;
		kp.nst = nst;
		kp.base = nst + nf;
		kp.xy = nullptr;
		kp.boxes = nullptr;
		const dim3 rgrid((unsigned)((pl.scan_h + 3) / 4), (unsigned)nf);
		HIPCHK(hipMemcpyAsync(thr, hthr.data(), sizeof(int) * nf, hipMemcpyHostToDevice, s));
		hipLaunchKernelGGL(k_findstar_peak, rgrid, dim3(256), 0, s, kp);
		HIPCHK(hipGetLastError());
		hipLaunchKernelGGL(k_findstar_scan, dim3((unsigned)nf), dim3(64), 0, s, rows, pl.scan_h, tot);
		HIPCHK(hipGetLastError());
		HIPCHK(hipMemcpyAsync(htot.data(), tot, sizeof(uint32_t) * nf, hipMemcpyDeviceToHost, s));
		HIPCHK(hipStreamSynchronize(s));
		uint64_t total = 0, most = 0;
		for (int f = 0; f < nf; f++) {
			rec[f].ncand = htot[f];
			rec[f].nstored = std::min<int64_t>(htot[f], pl.max_candidates);
			hnst[f] = (uint64_t)rec[f].nstored;
			hnst[nf + f] = total;
			total += hnst[f];
			most = std::max(most, hnst[f]);
		}
		if (total == 0)
			continue;
		const size_t xy_bytes = sg_up16(total * 2 * sizeof(int32_t));
		const size_t box_bytes = boxes ? total * (size_t)pl.box_elems * sizeof(uint16_t) : 0;
		HIPCHK(ensure(dv.fs_out, xy_bytes + box_bytes));
		kp.xy = (int *)dv.fs_out.p;
		kp.boxes = (uint16_t *)((char *)dv.fs_out.p + xy_bytes);
		HIPCHK(hipMemcpyAsync(nst, hnst.data(), 2 * sizeof(uint64_t) * nf, hipMemcpyHostToDevice, s));
		hipLaunchKernelGGL(k_findstar_emit, rgrid, dim3(256), 0, s, kp);
		HIPCHK(hipGetLastError());
		if (boxes) {
			hipLaunchKernelGGL(k_findstar_boxes, dim3((unsigned)((most + 3) / 4), (unsigned)nf), dim3(256), 0, s, kp);
			HIPCHK(hipGetLastError());
		}
		/* each frame's stored entries straight into the caller's arrays */
		for (int f = 0; f < nf && cand_xy; f++) {
			const size_t at = hnst[nf + f], n = hnst[f], slot = (size_t)(f0 + f) * pl.max_candidates;
			if (!n)
				continue;
			HIPCHK(hipMemcpyAsync(cand_xy + slot * 2, kp.xy + at * 2, n * 2 * sizeof(int32_t), hipMemcpyDeviceToHost, s));
			if (boxes)
				HIPCHK(hipMemcpyAsync(boxes + slot * (size_t)pl.box_elems, kp.boxes + at * (size_t)pl.box_elems,
						n * (size_t)pl.box_elems * sizeof(uint16_t), hipMemcpyDeviceToHost, s));
		}
		if (fp) {
			/* the chunk's fit block: medians, star counts, candidate records, compact stars */
			const size_t o_bg = 0, o_ns = o_bg + sg_up16(sizeof(double) * nf), o_cd = o_ns + sg_up16(sizeof(int) * nf);
			const size_t o_st = o_cd + sg_up16(total * sizeof(sg_starfit_cand));
			HIPCHK(ensure(dv.fs_fit, o_st + sg_up16(total * sizeof(sg_star))));
			char *fb = (char *)dv.fs_fit.p;
			for (int f = 0; f < nf; f++)
				hmed[f] = rec[f].median;
			HIPCHK(hipMemcpyAsync(fb + o_bg, hmed.data(), sizeof(double) * nf, hipMemcpyHostToDevice, s));
			SgFitParams q;
			q.img = lay;
			q.fstride = frame_stride;
			q.W = W;
			q.H = H;
			q.r = pl.r;
			q.max_stars = fp->max_stars;
			q.nst = nst;
			q.base = nst + nf;
			q.xy = kp.xy;
			q.bg = (const double *)(fb + o_bg);
			q.norm = fp->norm;
			q.scale_x = fp->scale_x;
			q.scale_y = fp->scale_y;
			q.roundness = fp->roundness;
			q.cands = (sg_starfit_cand *)(fb + o_cd);
			q.stars = (sg_star *)(fb + o_st);
			q.nstars = (int *)(fb + o_ns);
			hipLaunchKernelGGL(k_starfit_fit, dim3(sgs_grid_x(most), (unsigned)nf), dim3(64 * SGS_WAVES), fp->lds_bytes, s, q);
			HIPCHK(hipGetLastError());
			hipLaunchKernelGGL(k_starfit_select, dim3((unsigned)nf), dim3(64), 0, s, q);
			HIPCHK(hipGetLastError());
			HIPCHK(hipMemcpyAsync(nstars + f0, q.nstars, sizeof(int) * nf, hipMemcpyDeviceToHost, s));
			HIPCHK(hipStreamSynchronize(s));
			for (int f = 0; f < nf; f++) {
				const size_t at = hnst[nf + f], n = hnst[f];
				if (nstars[f0 + f] > 0)
					HIPCHK(hipMemcpyAsync(stars + (size_t)(f0 + f) * fp->max_stars, q.stars + at,
							(size_t)nstars[f0 + f] * sizeof(sg_star), hipMemcpyDeviceToHost, s));
				if (cands && n)
					HIPCHK(hipMemcpyAsync(cands + (size_t)(f0 + f) * pl.max_candidates, q.cands + at,
							n * sizeof(sg_starfit_cand), hipMemcpyDeviceToHost, s));
			}
		}
		HIPCHK(hipStreamSynchronize(s));
		for (int f = 0; fp && f < nf; f++) {	/* sort_stars: ascending mag; ties by candidate (the serial order) */
			sg_star *b = stars + (size_t)(f0 + f) * fp->max_stars;
			std::sort(b, b + nstars[f0 + f], [](const sg_star &u, const sg_star &v) {
				return u.mag < v.mag || (u.mag == v.mag && u.cand < v.cand);
			});
		}
	}
	return SG_OK;
}

extern "C" int sg_findstar_device(sg_ctx *ctx, int dev_index, const sg_findstar_desc *desc, const uint16_t *d_frames,
		int nframes, int64_t frame_stride, sg_findstar_frame *per_frame, int32_t *cand_xy, uint16_t *boxes,
		uint16_t *d_wave, void *stream) {
	if (!sg_dev_ok(ctx, dev_index))
		return SG_ERR_GENERIC;
	SgFindstarPlan pl;
	int rc = sg_findstar_plan(desc, pl);
	if (rc != SG_OK)
		return set_err(ctx, rc, "%s", pl.err);
	if (!d_frames || nframes < 1 || !per_frame || frame_stride < 0 || (pl.max_candidates > 0 && !cand_xy))
		return set_err(ctx, SG_ERR_GENERIC, "findstar: missing frames, records or candidate array%s", "");
	return sgf_run(ctx, dev_index, pl, d_frames, nframes, frame_stride, per_frame, cand_xy, boxes, d_wave, stream, nullptr,
			nullptr, nullptr, nullptr);
}

static int sgs_check(sg_ctx *ctx, const sg_starfit_desc *desc, SgStarfitPlan &fp, const void *frames, int nframes,
		const sg_findstar_frame *per_frame, const int32_t *nstars, const sg_star *stars, const sg_starfit_cand *cands) {
	const int rc = sg_starfit_plan(desc, fp);
	if (rc != SG_OK)
		return set_err(ctx, rc, "%s", fp.err);
	if (!frames || nframes < 1 || !per_frame || !nstars || (fp.max_stars > 0 && !stars) ||
			(fp.want_candidates && fp.find.max_candidates > 0 && !cands))
		return set_err(ctx, SG_ERR_GENERIC, "starfit: missing frames, records, star or candidate array%s", "");
	return SG_OK;
}

extern "C" int sg_findstar_fit_device(sg_ctx *ctx, int dev_index, const sg_starfit_desc *desc, const uint16_t *d_frames,
		int nframes, int64_t frame_stride, sg_findstar_frame *per_frame, int32_t *nstars, sg_star *stars,
		sg_starfit_cand *cands, void *stream) {
	if (!sg_dev_ok(ctx, dev_index))
		return SG_ERR_GENERIC;
	SgStarfitPlan fp;
	const int rc = sgs_check(ctx, desc, fp, d_frames, nframes, per_frame, nstars, stars, cands);
	if (rc != SG_OK)
		return rc;
	if (frame_stride < 0)
		return set_err(ctx, SG_ERR_GENERIC, "starfit: negative frame stride%s", "");
	return sgf_run(ctx, dev_index, fp.find, d_frames, nframes, frame_stride, per_frame, nullptr, nullptr, nullptr, stream,
			&fp, nstars, stars, fp.want_candidates ? cands : nullptr);
}

/* the host entries: batches of frames through sgf_run; the plane, when asked for, follows the batch's frames */
static int sgf_host(sg_ctx *ctx, const SgFindstarPlan &pl, const uint16_t *frames, int nframes, sg_findstar_frame *per_frame,
		int32_t *cand_xy, uint16_t *boxes, uint16_t *wave, const SgStarfitPlan *fp, int32_t *nstars, sg_star *stars,
		sg_starfit_cand *cands) {
	const size_t npix = (size_t)pl.W * pl.H, maxc = (size_t)pl.max_candidates;
	SgHostBatches hb(ctx);
	HIPCHK(hb.begin(nframes, npix * pl.C, SG_HOST_BUDGET_1G, 0, 0, wave ? npix : 0));
	while (hb.next()) {
		const size_t f0 = (size_t)hb.f0;
		HIPCHK(hb.upload(frames));
		const int rc = sgf_run(ctx, 0, pl, hb.d, hb.nf, 0, per_frame + f0, cand_xy ? cand_xy + f0 * maxc * 2 : nullptr,
				boxes ? boxes + f0 * maxc * (size_t)pl.box_elems : nullptr, hb.tail, nullptr, fp, nstars ? nstars + f0 : nullptr,
				stars ? stars + f0 * (size_t)fp->max_stars : nullptr, cands ? cands + f0 * maxc : nullptr);
		if (rc != SG_OK)
			return rc;
		if (wave) {
			HIPCHK(hipMemcpyAsync(wave + f0 * npix, hb.tail, (size_t)hb.nf * npix * sizeof(uint16_t), hipMemcpyDeviceToHost,
					hb.dv.stream));
			HIPCHK(hipStreamSynchronize(hb.dv.stream));
		}
	}
	return SG_OK;
}

extern "C" int sg_findstar_fit(sg_ctx *ctx, const sg_starfit_desc *desc, const uint16_t *frames, int nframes,
		sg_findstar_frame *per_frame, int32_t *nstars, sg_star *stars, sg_starfit_cand *cands) {
	if (!ctx || ctx->dev.empty())
		return SG_ERR_GENERIC;
	SgStarfitPlan fp;
	int rc = sgs_check(ctx, desc, fp, frames, nframes, per_frame, nstars, stars, cands);
	if (rc != SG_OK)
		return rc;
	return sgf_host(ctx, fp.find, frames, nframes, per_frame, nullptr, nullptr, nullptr, &fp, nstars, stars,
			fp.want_candidates ? cands : nullptr);
}

extern "C" int sg_findstar(sg_ctx *ctx, const sg_findstar_desc *desc, const uint16_t *frames, int nframes,
		sg_findstar_frame *per_frame, int32_t *cand_xy, uint16_t *boxes, uint16_t *wave) {
	if (!ctx || ctx->dev.empty())
		return SG_ERR_GENERIC;
	SgFindstarPlan pl;
	int rc = sg_findstar_plan(desc, pl);
	if (rc != SG_OK)
		return set_err(ctx, rc, "%s", pl.err);
	if (!frames || nframes < 1 || !per_frame || (pl.max_candidates > 0 && !cand_xy))
		return set_err(ctx, SG_ERR_GENERIC, "findstar: missing frames, records or candidate array%s", "");
	return sgf_host(ctx, pl, frames, nframes, per_frame, cand_xy, boxes, wave, nullptr, nullptr, nullptr, nullptr);
}
