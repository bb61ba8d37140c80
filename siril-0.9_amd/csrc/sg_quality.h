/*
 * sg_quality.h - the rule of QualityEstimate(fit, layer, QUALTYPE_NORMAL)
 * (src/algos/quality.c:46-218) for a W x H plane, host + device, shared by the kernels of
 * sg_quality.hip and by the stand-alone program of tests/test_quality_cpu.py, which runs both
 * routes on the CPU with these functions and the index functions of sg_quality_plan.hpp.
 *
 * Only subsample 3 contributes: the later subsamples are weighted by the integer quotient
 * (3 * 3) / (subsample * subsample) = 0 (quality.c:192-194), and their q is finite, so they add
 * +-0 to the sum.  What is left, on the plane in memory order:
 *   1. xs = (W - 1) / 3, ys = (H - 1) / 3; xs < 2 || ys < 2: the loop breaks at once, sqrt(0) = 0.
 *   2. sample (j, i) = the sum of rows 3j .. 3j + 2, columns 3i .. 3i + 2, / 9 (integers).
 *   3. max = the largest sample of rows 1 .. ys - 2 with 0 < v < 65530: the maxp[] insertion
 *      stores v in every slot behind the first, so its upper three slots all hold the running
 *      maximum.
 *   4. max > 0: v = (unsigned)((double)v * (60000.0 / (double)max)), clamped at 65535, in fp64.
 *   5. smoothed = the 3 x 3 sum / 9 (integers), the border ring 0.
 *   6. xb = (int)(xs * 0.1) + 1, yb = (int)(ys * 0.1) + 1.  A pixel inside the margins
 *      (xb <= x < xs - xb, yb <= y < ys - yb) whose smoothed value is >= 40 << 8 flags its 3 x 3
 *      neighbourhood; a flagged pixel inside the margins adds (s - right)^2 + (s - below)^2 and
 *      counts.
 *   7. sqrt(val / pixels / 10); NaN (the reference's sqrt(-1)) when no pixel passed the threshold.
 * The sums are integers, converted once: equal to the reference's double accumulation while
 * val < 2^53.
 */
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define SGQ_HD __host__ __device__ static inline
#else
#define SGQ_HD static inline
#endif

#define SGQ_SUB 3		/* QSUBSAMPLE_MIN */
#define SGQ_VMAX 65530		/* a sample takes part in the maximum below this */
#define SGQ_TARGET 60000.0
#define SGQ_THRESHOLD (40 << 8)	/* THRESHOLD << 8 */

struct sgq_geom {
	int xs, ys;	/* samples across and down */
	int xb, yb;	/* margins of the gradient */
};

SGQ_HD sgq_geom sgq_geometry(int W, int H) {
	sgq_geom g;
	g.xs = (W - 1) / SGQ_SUB;
	g.ys = (H - 1) / SGQ_SUB;
	g.xb = (int)((double)g.xs * 0.1) + 1;
	g.yb = (int)((double)g.ys * 0.1) + 1;
	return g;
}

/* a u16 plane or tile seen in plane coordinates: element (x, y) at p[(y - y0) * w + (x - x0)] */
struct sgq_view {
	const uint16_t *p;
	int w, x0, y0;
#if defined(__HIPCC__)
	__host__ __device__
#endif
	uint32_t operator()(int x, int y) const {
		return p[(y - y0) * w + (x - x0)];
	}
};

/* SubSample(ptr, width, 3, 3): p points at row 3j, column 3i */
SGQ_HD uint32_t sgq_sample(const uint16_t *p, int64_t row_pitch) {
	uint32_t v = 0;
	for (int r = 0; r < SGQ_SUB; r++, p += row_pitch)
		v += (uint32_t)p[0] + (uint32_t)p[1] + (uint32_t)p[2];
	return v / (SGQ_SUB * SGQ_SUB);
}

/* Samples are taken two at a time: slot k of sample row y holds samples 2k and 2k + 1 (the second
 * only if 2k + 1 < xs).  Their six columns start at element 6k, so when every row of the frame
 * starts on a dword (`aligned`: the base address, the row pitch and the frame pitch are even in
 * elements) a full slot is three dword loads per row instead of six 2-byte ones.  Returns the
 * number of samples written to v[]. */
SGQ_HD bool sgq_rows_aligned(const uint16_t *frames, int64_t frame_pitch, int64_t row_pitch) {
	return !((uintptr_t)frames & 3) && !(frame_pitch & 1) && !(row_pitch & 1);
}

SGQ_HD int sgq_sample_slot(const uint16_t *img, int64_t row_pitch, bool aligned, int xs, int y, int k, uint32_t v[2]) {
	const uint16_t *p = img + (int64_t)(SGQ_SUB * y) * row_pitch + 2 * SGQ_SUB * k;
	if (2 * k + 1 >= xs) {
		v[0] = sgq_sample(p, row_pitch);
		return 1;
	}
	if (!aligned) {
		v[0] = sgq_sample(p, row_pitch);
		v[1] = sgq_sample(p + SGQ_SUB, row_pitch);
		return 2;
	}
	uint32_t a = 0, b = 0;
	for (int r = 0; r < SGQ_SUB; r++, p += row_pitch) {
		const uint32_t *d = (const uint32_t *)p;	/* elements 0 1 | 2 3 | 4 5, little endian */
		const uint32_t d0 = d[0], d1 = d[1], d2 = d[2];
		a += (d0 & 0xffffu) + (d0 >> 16) + (d1 & 0xffffu);
		b += (d1 >> 16) + (d2 & 0xffffu) + (d2 >> 16);
	}
	v[0] = a / (SGQ_SUB * SGQ_SUB);
	v[1] = b / (SGQ_SUB * SGQ_SUB);
	return 2;
}

/* what sample v of row j offers to the maximum (0 = nothing) */
SGQ_HD uint32_t sgq_max_term(uint32_t v, int j, int ys) {
	return (j >= 1 && j <= ys - 2 && v < SGQ_VMAX) ? v : 0u;
}

SGQ_HD double sgq_mult(uint32_t max) {
	return SGQ_TARGET / (double)max;
}

/* step 4; mult = sgq_mult(max), unused when max == 0 */
SGQ_HD uint32_t sgq_stretch(uint32_t v, uint32_t max, double mult) {
	if (max == 0)
		return v;
	uint32_t s = (uint32_t)((double)v * mult);	/* at most 65535 * 60000 < 2^32 */
	return s > 65535u ? 65535u : s;
}

/* step 5 at (x, y); st(x, y) gives the stretched sample, asked only inside the plane */
template <class G> SGQ_HD uint32_t sgq_smooth(const G &st, int x, int y, int xs, int ys) {
	if (x < 1 || y < 1 || x > xs - 2 || y > ys - 2)
		return 0;
	uint32_t v = 0;
	for (int dy = -1; dy <= 1; dy++)
		for (int dx = -1; dx <= 1; dx++)
			v += st(x + dx, y + dy);
	return v / 9;
}

SGQ_HD bool sgq_inside(int x, int y, const sgq_geom &g) {
	return x >= g.xb && x < g.xs - g.xb && y >= g.yb && y < g.ys - g.yb;
}

/* step 6 at (x, y); sm(x, y) gives the smoothed value, asked only inside the plane (the margins
 * are at least 1, so every neighbour of a pixel inside them is).  Returns whether the pixel
 * counts, and its term. */
template <class G> SGQ_HD bool sgq_gradient(const G &sm, int x, int y, const sgq_geom &g, uint64_t *term) {
	if (!sgq_inside(x, y, g))
		return false;
	bool flagged = false;
	for (int dy = -1; dy <= 1; dy++)
		for (int dx = -1; dx <= 1; dx++)
			if (sgq_inside(x + dx, y + dy, g) && sm(x + dx, y + dy) >= (uint32_t)SGQ_THRESHOLD)
				flagged = true;
	if (!flagged)
		return false;
	const int64_t c = (int64_t)sm(x, y), d1 = c - (int64_t)sm(x + 1, y), d2 = c - (int64_t)sm(x, y + 1);
	*term = (uint64_t)(d1 * d1 + d2 * d2);
	return true;
}

/* The tiled route's gradient pass, element by element, as k_qest_gradient and the CPU program run
 * it: tile (tx0, ty0) covers SGQ_TILE_X x SGQ_TILE_Y samples; its stretched tile starts 2 before
 * the origin, its smoothed tile 1 before. */
#define SGQ_TILE_X 64
#define SGQ_TILE_Y 16
#define SGQ_ST_W (SGQ_TILE_X + 4)
#define SGQ_ST_H (SGQ_TILE_Y + 4)
#define SGQ_SM_W (SGQ_TILE_X + 2)
#define SGQ_SM_H (SGQ_TILE_Y + 2)

/* element i of the stretched tile, from the frame's sample plane [ys][xs]; 0 outside the plane */
SGQ_HD uint16_t sgq_tile_stretched(const uint16_t *plane, int xs, int ys, int tx0, int ty0, int i, uint32_t max, double mult) {
	const int ly = i / SGQ_ST_W, x = tx0 - 2 + (i - ly * SGQ_ST_W), y = ty0 - 2 + ly;
	if (x < 0 || x >= xs || y < 0 || y >= ys)
		return 0;
	return (uint16_t)sgq_stretch(plane[(int64_t)y * xs + x], max, mult);
}

/* element i of the smoothed tile, from the stretched tile; 0 outside the plane's interior */
SGQ_HD uint16_t sgq_tile_smoothed(const uint16_t *st_tile, int xs, int ys, int tx0, int ty0, int i) {
	const int ly = i / SGQ_SM_W, x = tx0 - 1 + (i - ly * SGQ_SM_W), y = ty0 - 1 + ly;
	const sgq_view st = {st_tile, SGQ_ST_W, tx0 - 2, ty0 - 2};
	return (uint16_t)sgq_smooth(st, x, y, xs, ys);
}

/* sample i of the tile, from the smoothed tile: whether it counts, and its term */
SGQ_HD bool sgq_tile_term(const uint16_t *sm_tile, const sgq_geom &g, int tx0, int ty0, int i, uint64_t *term) {
	const int ly = i / SGQ_TILE_X, x = tx0 + (i - ly * SGQ_TILE_X), y = ty0 + ly;
	const sgq_view sm = {sm_tile, SGQ_SM_W, tx0 - 1, ty0 - 1};
	return sgq_gradient(sm, x, y, g, term);
}

/* a tile without a pixel inside the margins adds nothing */
SGQ_HD bool sgq_tile_idle(const sgq_geom &g, int tx0, int ty0) {
	return tx0 >= g.xs - g.xb || tx0 + SGQ_TILE_X <= g.xb || ty0 >= g.ys - g.yb || ty0 + SGQ_TILE_Y <= g.yb;
}

/* step 7 */
SGQ_HD double sgq_finish(uint64_t val, uint64_t pixels) {
	if (pixels == 0)
		return (double)NAN;
	double q = (double)val / (double)pixels;
	q = q / 10;
	return sqrt(q);
}
