/*
 * sg_findstar_plan.hpp - the host-only plan of a star-candidate call (include/sirilgpu.h,
 * sg_findstar*): everything peaker (src/algos/star_finder.c:103-255) decides on the host before
 * and between its whole-image passes, with no HIP in it, so tests/test_findstar_plan_cpu.py builds
 * and checks it without a GPU:
 *   - the argument checks (each before any device work);
 *   - the wavelet / no-wavelet decision (wavelet_transform_data, src/algos/transform.c:194-201);
 *   - the scan rectangle of the peak test (:176-178), which may be empty;
 *   - the tile grid of the fused two-pass smoothing kernel, its halo and LDS bytes, and the
 *     tile's passes themselves (sgf_tile_*, host + device: the kernel's index arithmetic);
 *   - the scratch sizes per frame and the frames per chunk;
 *   - the host finish of Compute_threshold (:39-57): sigma from the exact integer sums and the
 *     WORD conversion of the threshold.
 */
#pragma once
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include "../../include/sirilgpu.h"
#include "sg_prepro_plan.hpp"

#define SGF_TILE_W 64		/* output tile of k_findstar_plane (columns, rows) */
#define SGF_TILE_H 32
#define SGF_HALO 6		/* 2 * Step of pass 1 (Step 1) + 2 * Step of pass 2 (Step 2) */
#define SGF_HALO2 4		/* pass-1 values pass 2 reads around the tile: 2 * Step of pass 2 */
#define SGF_MIN_SIDE 32		/* pow(2, Nbr_Plan + 2) for Nbr_Plan = 3 */
#define SGF_BINS 65536
#define SGF_PLANE_BUDGET ((int64_t)1 << 29)	/* pixels of scratch plane per chunk of frames (1 GiB) */

/* shared by the host plan and the kernels */
#if defined(__HIPCC__)
#define SGF_HD __host__ __device__ static inline
#else
#define SGF_HD static inline
#endif

/* one pixel of pave_2d_bspline_smooth (pave.c:250-279), the operands as the source has them:
 * r3 / r1 / r0 / r2 / r4 are the rows indi3 (i - 2 Step), indi1 (i - Step), i, indi2, indi4 and
 * j3 / j1 / j / j2 / j4 the columns likewise.  Float adds in source order inside each group, the
 * group sum times its double constant, the six products added in double left to right, the result
 * rounded to float.  No contraction is possible: every product is exact. */
template <typename T>
SGF_HD float sgf_bspline(const T *r3, const T *r1, const T *r0, const T *r2, const T *r4, int j3, int j1, int j,
		int j2, int j4) {
	const float g1 = (float)r3[j3] + (float)r3[j4] + (float)r4[j3] + (float)r4[j4];
	const float g2 = (float)r4[j2] + (float)r3[j2] + (float)r4[j1] + (float)r3[j1] + (float)r2[j3] + (float)r2[j4] +
			(float)r1[j3] + (float)r1[j4];
	const float g3 = (float)r3[j] + (float)r4[j] + (float)r0[j3] + (float)r0[j4];
	const float g4 = (float)r1[j1] + (float)r1[j2] + (float)r2[j1] + (float)r2[j2];
	const float g5 = (float)r1[j] + (float)r2[j] + (float)r0[j1] + (float)r0[j2];
	return (float)(0.00390625 * g1 + 0.015625 * g2 + 0.0234375 * g3 + 0.06250 * g4 + 0.09375 * g5 +
			0.140625 * (float)r0[j]);
}

/* test_ind (pave.c:88-102) */
SGF_HD int sgf_clamp(int ind, int n) {
	return ind < 0 ? 0 : (ind >= n ? n - 1 : ind);
}

/*
 * The fused two-pass tile of k_findstar_plane, shared with the host so the
 * index arithmetic is checked there: s_in is the u16 tile with a halo of SGF_HALO loaded through the
 * clamp (so pass 1 indexes it plainly), s_mid the pass-1 floats with a halo of SGF_HALO2, defined at
 * in-image positions only (pass 2 clamps its indices first, then subtracts the tile's origin).
 */
#define SGF_IN_W (SGF_TILE_W + 2 * SGF_HALO)
#define SGF_IN_H (SGF_TILE_H + 2 * SGF_HALO)
#define SGF_MID_W (SGF_TILE_W + 2 * SGF_HALO2)
#define SGF_MID_H (SGF_TILE_H + 2 * SGF_HALO2)

/* s_in[idx], idx in [0, SGF_IN_H * SGF_IN_W) */
SGF_HD uint16_t sgf_tile_load(int idx, const uint16_t *img, int W, int H, int tx0, int ty0) {
	const int ly = idx / SGF_IN_W, lx = idx - ly * SGF_IN_W;
	const int gy = sgf_clamp(ty0 - SGF_HALO + ly, H), gx = sgf_clamp(tx0 - SGF_HALO + lx, W);
	return img[(int64_t)gy * W + gx];
}

/* Both passes walk a column strip: the rows a strip's pixels share are read from LDS once (9 rows
 * of 5 for 5 pixels of pass 1, 16 rows of 5 for 8 pixels of pass 2, instead of 25 reads a pixel). */
#define SGF_P1_ROWS 5		/* pass-1 strip: SGF_MID_H / 5 strips a column */
#define SGF_P1_ITEMS ((SGF_MID_H / SGF_P1_ROWS) * SGF_MID_W)
#define SGF_P2_ROWS 8		/* pass-2 strip: SGF_TILE_H / 8 strips a column, one per thread of 256 */
#define SGF_P2_ITEMS ((SGF_TILE_H / SGF_P2_ROWS) * SGF_TILE_W)

/* pass 1 (Step 1), strip `item` in [0, SGF_P1_ITEMS): s_mid at its in-image positions */
SGF_HD void sgf_tile_pass1(int item, const uint16_t *s_in, float *s_mid, int W, int H, int tx0, int ty0) {
	const int strip = item / SGF_MID_W, lx = item - strip * SGF_MID_W, ly0 = strip * SGF_P1_ROWS;
	const int gx = tx0 - SGF_HALO2 + lx, gy0 = ty0 - SGF_HALO2 + ly0;
	if (gx < 0 || gx >= W)
		return;
	float R[SGF_P1_ROWS + 4][5];	/* s_in rows ly0 .. ly0 + 8 (centre row ly + 2), columns lx .. lx + 4 */
#pragma unroll
	for (int t = 0; t < SGF_P1_ROWS + 4; t++)
#pragma unroll
		for (int c = 0; c < 5; c++)
			R[t][c] = (float)s_in[(ly0 + t) * SGF_IN_W + lx + c];
#pragma unroll
	for (int u = 0; u < SGF_P1_ROWS; u++)
		if (gy0 + u >= 0 && gy0 + u < H)
			s_mid[(ly0 + u) * SGF_MID_W + lx] = sgf_bspline(R[u], R[u + 1], R[u + 2], R[u + 3], R[u + 4], 0, 1, 2, 3, 4);
}

/* pass 2 (Step 2), strip `item` in [0, SGF_P2_ITEMS): v[u] is the pixel (*gx, *gy0 + u) for u below
 * the returned count (0 when the strip lies outside the image).  The clamp goes on the image
 * indices, then the tile's origin is subtracted. */
SGF_HD int sgf_tile_pass2(int item, const float *s_mid, int W, int H, int tx0, int ty0, int *gy0_out, int *gx_out,
		float v[SGF_P2_ROWS]) {
	const int ox = item % SGF_TILE_W, gx = tx0 + ox, gy0 = ty0 + (item / SGF_TILE_W) * SGF_P2_ROWS;
	if (gx >= W || gy0 >= H)
		return 0;
	const int by = ty0 - SGF_HALO2, bx = tx0 - SGF_HALO2;
	const int col[5] = {sgf_clamp(gx - 4, W) - bx, sgf_clamp(gx - 2, W) - bx, gx - bx, sgf_clamp(gx + 2, W) - bx,
		sgf_clamp(gx + 4, W) - bx};
	float R[SGF_P2_ROWS + 8][5];	/* image rows clamp(gy0 - 4 + t) */
#pragma unroll
	for (int t = 0; t < SGF_P2_ROWS + 8; t++) {
		const float *row = s_mid + (sgf_clamp(gy0 - 4 + t, H) - by) * SGF_MID_W;
#pragma unroll
		for (int c = 0; c < 5; c++)
			R[t][c] = row[col[c]];
	}
#pragma unroll
	for (int u = 0; u < SGF_P2_ROWS; u++)
		v[u] = sgf_bspline(R[u], R[u + 2], R[u + 4], R[u + 6], R[u + 8], 0, 1, 2, 3, 4);
	*gy0_out = gy0;
	*gx_out = gx;
	return H - gy0 < SGF_P2_ROWS ? H - gy0 : SGF_P2_ROWS;
}

struct SgFindstarPlan {
	int W = 0, H = 0, C = 0, layer = 0, r = 0, max_candidates = 0;
	double k = 0.;
	int wavelet = 0;		/* 0: the detection plane is the unsmoothed image */
	int ax0 = 0, ay0 = 0, ax1 = 0, ay1 = 0;	/* area, display coordinates */
	int sx0 = 0, sy0 = 0, scan_w = 0, scan_h = 0;	/* x in [sx0, sx0 + scan_w), y in [sy0, sy0 + scan_h) */
	int tiles_x = 0, tiles_y = 0, halo = SGF_HALO;
	int in_w = 0, in_h = 0, mid_w = 0, mid_h = 0;	/* LDS tiles: u16 input, pass-1 floats */
	size_t lds_bytes = 0;
	int mask_words = 0;		/* 64-bit candidate masks per scanned row */
	int64_t box_elems = 0;		/* 2r * 2r */
	size_t hist_bytes = 0, stat_bytes = 0, mask_bytes = 0, rows_bytes = 0, plane_bytes = 0;	/* per frame */
	char err[256] = "";
};

static inline int sgf_fail(SgFindstarPlan &p, int code, const char *msg) {
	snprintf(p.err, sizeof p.err, "%s", msg);
	return code;
}

static inline int sg_findstar_plan(const sg_findstar_desc *d, SgFindstarPlan &p) {
	p = SgFindstarPlan();
	if (!d)
		return sgf_fail(p, SG_ERR_GENERIC, "no descriptor");
	if (d->width <= 0 || d->height <= 0 || d->nb_layers <= 0)
		return sgf_fail(p, SG_ERR_SIZE, "findstar: width, height and nb_layers must be positive");
	if ((int64_t)d->width * d->height >= (1ll << 31))
		return sgf_fail(p, SG_ERR_SIZE, "findstar: a plane of 2^31 pixels or more");
	if (d->layer < 0 || d->layer >= d->nb_layers)
		return sgf_fail(p, SG_ERR_SIZE, "findstar: layer outside [0, nb_layers)");
	if (d->use_area) {
		const sg_rect &a = d->area;
		if (a.x < 0 || a.y < 0 || a.w < 0 || a.h < 0 || (int64_t)a.x + a.w > d->width || (int64_t)a.y + a.h > d->height)
			return sgf_fail(p, SG_ERR_SIZE, "findstar: the area is not inside the image (the reference reads out of bounds)");
	}
	if (d->radius < 1)
		return sgf_fail(p, SG_ERR_GENERIC, "findstar: radius below 1 (the 3x3 peak test would leave the image)");
	if (!(d->sigma >= 0.) || !isfinite(d->sigma))
		return sgf_fail(p, SG_ERR_GENERIC, "findstar: sigma negative or not finite");
	if (d->max_candidates < 0)
		return sgf_fail(p, SG_ERR_GENERIC, "findstar: max_candidates negative");
	p.W = d->width;
	p.H = d->height;
	p.C = d->nb_layers;
	p.layer = d->layer;
	p.r = d->radius;
	p.k = d->sigma;
	p.max_candidates = d->max_candidates;
	p.wavelet = (p.W < p.H ? p.W : p.H) >= SGF_MIN_SIDE;
	p.ax0 = d->use_area ? d->area.x : 0;
	p.ay0 = d->use_area ? d->area.y : 0;
	p.ax1 = d->use_area ? d->area.x + d->area.w : p.W;
	p.ay1 = d->use_area ? d->area.y + d->area.h : p.H;
	const int64_t sw = (int64_t)p.ax1 - p.ax0 - 2 * (int64_t)p.r, sh = (int64_t)p.ay1 - p.ay0 - 2 * (int64_t)p.r;
	if (sw > 0 && sh > 0) {
		p.sx0 = p.ax0 + p.r;
		p.sy0 = p.ay0 + p.r;
		p.scan_w = (int)sw;
		p.scan_h = (int)sh;
		p.box_elems = 4 * (int64_t)p.r * p.r;
	}
	p.tiles_x = (p.W + SGF_TILE_W - 1) / SGF_TILE_W;
	p.tiles_y = (p.H + SGF_TILE_H - 1) / SGF_TILE_H;
	p.in_w = SGF_IN_W;
	p.in_h = SGF_IN_H;
	p.mid_w = SGF_MID_W;
	p.mid_h = SGF_MID_H;
	p.lds_bytes = (size_t)p.in_w * p.in_h * sizeof(uint16_t) + (size_t)p.mid_w * p.mid_h * sizeof(float);
	p.mask_words = (p.scan_w + 63) / 64;
	p.hist_bytes = (size_t)SGF_BINS * sizeof(uint32_t);
	p.stat_bytes = 4 * sizeof(uint64_t);	/* ngood, sum, sum2, median */
	p.mask_bytes = (size_t)p.scan_h * p.mask_words * sizeof(uint64_t);
	p.rows_bytes = ((size_t)p.scan_h + 1) * sizeof(uint32_t);	/* row offsets, then the total */
	p.plane_bytes = (size_t)p.W * p.H * sizeof(uint16_t);
	return SG_OK;
}

/* frames per chunk: the scratch detection plane (when the caller keeps none) stays within 1 GiB,
 * the histograms within 64 MiB */
static inline int sgf_chunk_frames(const SgFindstarPlan &p, int nframes, int caller_plane) {
	int64_t c = 256;
	if (!caller_plane) {
		const int64_t fit = SGF_PLANE_BUDGET / ((int64_t)p.W * p.H);
		c = fit < c ? fit : c;
	}
	if (c < 1)
		c = 1;
	return nframes < c ? nframes : (int)c;
}

/* sigma of FnMeanSigma_ushort from the exact integer sums: valid when sum2 < 2^53, where every
 * partial sum of the reference's sequential double loop is an exact integer */
static inline int sgf_sums_exact(uint64_t sum2) {
	return sum2 < ((uint64_t)1 << 53);
}

static inline double sgf_sigma_sums(uint64_t n, uint64_t sum, uint64_t sum2) {
	if (n <= 1)
		return 0.0;
	const double xtemp = (double)sum / (double)n;
	return sqrt(((double)sum2 / (double)n) - (xtemp * xtemp));
}

/* sigma of FnMeanSigma_ushort as the reference sums it (sgp_mean_sigma_u16): the form for a plane
 * whose sum of squares passes 2^53, where the rounding order shows */
static inline double sgf_sigma_seq(const uint16_t *a, int64_t npix) {
	int64_t n;
	double mean, sigma;
	sgp_mean_sigma_u16(a, npix, &n, &mean, &sigma);
	return sigma;
}

/* (WORD)x of a double as x86-64 does it: cvttsd2si to int32 (0x80000000 when out of range or
 * NaN), the low 16 bits kept */
static inline uint16_t sgf_to_word(double x) {
	if (!(x > -2147483649.0 && x < 2147483648.0))
		return 0;
	return (uint16_t)(uint32_t)(int32_t)x;
}

/* threshold = (WORD) median + k * (WORD) sigma, stored to a WORD (star_finder.c:50); *wrapped
 * when the double is 65536 or more (undefined in C, the x86-64 result is kept) */
static inline uint16_t sgf_threshold(double median, double sigma, double k, int *wrapped) {
	const double t = (double)sgf_to_word(median) + k * (double)sgf_to_word(sigma);
	*wrapped = t >= 65536.0;
	return sgf_to_word(t);
}
