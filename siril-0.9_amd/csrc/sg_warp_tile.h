/*
 * sg_warp_tile.h - the per-pixel rule of the perspective warp (sg_warp.hip, k_warp) restated once,
 * host + device, and the source footprint of a destination tile.  Shared by k_warp_seq and by the
 * stand-alone program of tests/test_warp_plan_cpu.py, which runs both on the CPU.
 *
 * Per pixel (x, yd) of the destination in display (top-down) coordinates, with M = H^-1 and bw
 * OpenCV's block width:
 *   xb = (x / bw) * bw, x1 = x - xb;
 *   X0 = M0 xb + M1 yd + M2, Y0 = M3 xb + M4 yd + M5, W0 = M6 xb + M7 yd + M8   (double, this order)
 *   W = W0 + M6 x1;  W = W ? s / W : 0, s = 1 (nearest) or 32 (INTER_TAB_SIZE);
 *   fX = (X0 + M0 x1) W, fY = (Y0 + M3 x1) W, clamped to [INT_MIN, INT_MAX], rounded half to even;
 *   nearest: the source pixel (sat_short(X), sat_short(Y));
 *   else the K x K window starts at sat_short(X >> 5) - (K / 2 - 1) (and Y alike) and the
 *   coefficients are row (Y & 31) * 32 + (X & 31) of the table.
 * The float sums keep OpenCV's order: bilinear v0 w0 + v1 w1 + v2 w2 + v3 w3; cubic / Lanczos row
 * sums left to right added top to bottom when the window is inside the image, one running sum over
 * the taps inside it otherwise (a tap outside is skipped there, and reads 0 in the bilinear sum).
 *
 * Footprint.  In real arithmetic u = (M0 x + M1 y + M2) / (M6 x + M7 y + M8) and v alike are a
 * projective map; over a rectangle on which the denominator keeps one sign it maps the rectangle to
 * the convex quadrilateral of its four corners' images, so min / max of u and v over the tile are
 * attained at the corners.  What the kernel computes differs from the real value by:
 *   a. the double rounding of the sums: |X^ - X| <= 4 ulp-halves of SX = |M0| x + |M1| y + |M2|
 *      (four products of exactly represented integers, three sums), the same for W with SW; the
 *      quotient and the product add two more relative roundings.  With wmin = min |W| over the
 *      corners and umax = max |u|: |X^/W^ - u| <= E = 2^-50 ((SX + umax SW) / wmin + umax), 2^-50
 *      being eight half-ulps: twice the count above.  The corners evaluated here (plain sums, fewer
 *      roundings) are within E as well.  The tile takes the gather route unless E <= 1 / 128 for
 *      both coordinates, which also keeps the denominator away from 0;
 *   b. the 1/32 grid: X / 32 is within 1 / 64 of the rounded product.
 * So X / 32 lies within 1 / 64 + 2 E <= 1 / 32 of [umin^, umax^], the corners as computed.  The box
 * uses a slack of SGW_SLACK = 1 / 16, twice that:
 *   K > 1: columns floor(umin^ - 1/16) - (K / 2 - 1) .. floor(umax^ + 1/16) + K / 2;
 *   K = 1: round half to even of t lies in [ceil(t - 1/2), floor(t + 1/2)]:
 *          columns ceil(umin^ - 1/16 - 1/2) .. floor(umax^ + 1/16 + 1/2);
 * rows alike.  A corner beyond SGW_FAR source pixels (where the short saturation would move the
 * window) also takes the gather route.  The box is then cut to the image grown by K - 1 on every
 * side: a window with no tap inside the image is never read.  Correctness never rests on the box:
 * every pixel checks its own window against it and reads global memory when it is not inside.
 */
#pragma once
#include <limits.h>
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define SGW_HD __host__ __device__ static inline
#else
#define SGW_HD static inline
#endif

#if defined(__clang__)
#define SGW_UNROLL _Pragma("unroll")
#else
#define SGW_UNROLL
#endif

#define SGW_INTER_BITS 5
#define SGW_INTER_TAB 32
#define SGW_TILE_X 64		/* OpenCV's bw is 64 for out_height >= 16: a tile never straddles a block then */
#define SGW_TILE_Y 16
#define SGW_THREADS 256		/* a thread takes SGW_TILE_Y / 4 pixels of one column */
#define SGW_LDS_SAMPLES 8176	/* of u16: with the workgroup's sgw_box just below 16 KiB, a tenth of a CU's 160 KiB */
#define SGW_SLACK 0.0625
#define SGW_FAR 32000.0
#define SGW_ROUTE_GATHER 0
#define SGW_ROUTE_LDS 1

SGW_HD int sgw_ksize(int interp) {	/* taps per axis: 1 nearest, 2 linear / area, 4 cubic, 8 lanczos4 */
	return interp == 0 ? 1 : interp == 3 ? 4 : interp == 4 ? 8 : 2;
}

/* WarpPerspectiveInvoker's block width: BLOCK_SZ = 32, bh0 = min(16, height), bw0 = min(1024 / bh0, width) */
SGW_HD int sgw_block_width(int out_width, int out_height) {
	const int bh0 = out_height < 16 ? out_height : 16;
	const int bw0 = 1024 / bh0 < out_width ? 1024 / bh0 : out_width;
	return bw0 > 0 ? bw0 : 1;
}

SGW_HD uint16_t sgw_sat_u16(float v) {
	const float r = rintf(v);
	return r <= 0.f ? 0 : (r >= 65535.f ? 65535 : (uint16_t)r);
}

SGW_HD int sgw_sat_short(int v) {
	return v < -32768 ? -32768 : (v > 32767 ? 32767 : v);
}

SGW_HD int sgw_round(double v) {	/* cvRound of a value clamped to the int range */
	return (int)rint(fmax((double)INT_MIN, fmin((double)INT_MAX, v)));
}

struct sgw_coord {
	int sx, sy;	/* the window's first column and display row (K = 1: the pixel) */
	int tab;	/* row of the coefficient table (K = 1: 0) */
};

template <int K> SGW_HD sgw_coord sgw_coords(const double *M, int bw, int x, int yd) {
	const int xb = (x / bw) * bw, x1 = x - xb;
	const double X0 = M[0] * xb + M[1] * yd + M[2];
	const double Y0 = M[3] * xb + M[4] * yd + M[5];
	const double W0 = M[6] * xb + M[7] * yd + M[8];
	double W = W0 + M[6] * x1;
	sgw_coord c;
	if (K == 1) {
		W = W != 0.0 ? 1.0 / W : 0.0;
		c.sx = sgw_sat_short(sgw_round((X0 + M[0] * x1) * W));
		c.sy = sgw_sat_short(sgw_round((Y0 + M[3] * x1) * W));
		c.tab = 0;
	} else {
		W = W != 0.0 ? (double)SGW_INTER_TAB / W : 0.0;
		const int X = sgw_round((X0 + M[0] * x1) * W), Y = sgw_round((Y0 + M[3] * x1) * W);
		c.sx = sgw_sat_short(X >> SGW_INTER_BITS) - (K / 2 - 1);
		c.sy = sgw_sat_short(Y >> SGW_INTER_BITS) - (K / 2 - 1);
		c.tab = (Y & (SGW_INTER_TAB - 1)) * SGW_INTER_TAB + (X & (SGW_INTER_TAB - 1));
	}
	return c;
}

/* every tap of the window outside the W x H image: the pixel is the border value 0 */
template <int K> SGW_HD bool sgw_all_outside(const sgw_coord &c, int W, int H) {
	return c.sx >= W || c.sx + K - 1 < 0 || c.sy >= H || c.sy + K - 1 < 0;
}

/* the pixel from its window; src(x, y) is the sample of column x, display row y as a float, 0 outside
 * the image; wt = the K * K coefficients; not for a window sgw_all_outside */
template <int K, class S> SGW_HD uint16_t sgw_pixel(const S &src, const sgw_coord &c, const float *wt, int W, int H) {
	const int sx = c.sx, sy = c.sy;
	if (K == 1)
		return (uint16_t)src(sx, sy);
	if (K == 2) {
		const float sum = src(sx, sy) * wt[0] + src(sx + 1, sy) * wt[1] + src(sx, sy + 1) * wt[2] + src(sx + 1, sy + 1) * wt[3];
		return sgw_sat_u16(sum);
	}
	float sum = 0.f;
	if (sx >= 0 && sx + K <= W && sy >= 0 && sy + K <= H) {
		SGW_UNROLL
		for (int r = 0; r < K; r++) {
			float row = src(sx, sy + r) * wt[r * K];
			SGW_UNROLL
			for (int t = 1; t < K; t++)
				row = row + src(sx + t, sy + r) * wt[r * K + t];
			sum = r ? sum + row : row;
		}
	} else {
		for (int r = 0; r < K; r++) {
			if ((unsigned)(sy + r) >= (unsigned)H)
				continue;
			for (int t = 0; t < K; t++)
				if ((unsigned)(sx + t) < (unsigned)W)
					sum = sum + src(sx + t, sy + r) * wt[r * K + t];
		}
	}
	return sgw_sat_u16(sum);
}

/* the source box of a destination tile: columns x0 .. x1 and display rows y0 .. y1, both inclusive
 * (x1 < x0 or y1 < y0: no tap of the tile is inside the image), staged with `pitch` elements per row */
struct sgw_box {
	int route;
	int x0, y0, x1, y1;
	int pitch;
};

/* LDS row pitch in elements: an odd number of dwords, so that lanes stepping one row (a rotated
 * tile) step an odd number of the 32 banks a 2- or 4-byte read is spread over */
SGW_HD int sgw_lds_pitch(int w) {
	const int dw = (w + 1) / 2;
	return 2 * (dw | 1);
}

/* tile = destination columns tx0 .. tx1, display rows ty0 .. ty1 (inclusive, inside the output);
 * lds_samples = the staging budget in u16; force_gather = SG_WARP_ROUTE 1 */
SGW_HD sgw_box sgw_footprint(const double *M, int K, int tx0, int ty0, int tx1, int ty1, int W, int H, int lds_samples,
		int force_gather) {
	sgw_box b = {SGW_ROUTE_GATHER, 0, 0, -1, -1, 0};
	if (force_gather)
		return b;
	const int cx[4] = {tx0, tx1, tx0, tx1}, cy[4] = {ty0, ty0, ty1, ty1};
	double umin = 0, umax = 0, vmin = 0, vmax = 0, wmin = 0, sx = 0, sy = 0, sw = 0;
	int pos = 0, neg = 0;
	for (int k = 0; k < 4; k++) {
		const double x = cx[k], y = cy[k];
		const double w = M[6] * x + M[7] * y + M[8];
		const double u = (M[0] * x + M[1] * y + M[2]) / w, v = (M[3] * x + M[4] * y + M[5]) / w;
		pos += w > 0.0;
		neg += w < 0.0;
		if (!(fabs(u) <= SGW_FAR) || !(fabs(v) <= SGW_FAR))	/* also a NaN or an infinity */
			return b;
		const double aw = fabs(w);
		umin = k ? fmin(umin, u) : u;
		umax = k ? fmax(umax, u) : u;
		vmin = k ? fmin(vmin, v) : v;
		vmax = k ? fmax(vmax, v) : v;
		wmin = k ? fmin(wmin, aw) : aw;
		sx = fmax(sx, fabs(M[0]) * x + fabs(M[1]) * y + fabs(M[2]));
		sy = fmax(sy, fabs(M[3]) * x + fabs(M[4]) * y + fabs(M[5]));
		sw = fmax(sw, fabs(M[6]) * x + fabs(M[7]) * y + fabs(M[8]));
	}
	if (pos != 4 && neg != 4)	/* the horizon crosses the tile, or touches it */
		return b;
	const double eps = 8.8817841970012523e-16;	/* 2^-50 */
	const double ua = fmax(fabs(umin), fabs(umax)), va = fmax(fabs(vmin), fabs(vmax));
	const double eu = eps * ((sx + ua * sw) / wmin + ua), ev = eps * ((sy + va * sw) / wmin + va);
	if (!(eu <= 1.0 / 128) || !(ev <= 1.0 / 128))
		return b;
	int x0, x1, y0, y1;
	if (K == 1) {
		x0 = (int)ceil(umin - SGW_SLACK - 0.5);
		x1 = (int)floor(umax + SGW_SLACK + 0.5);
		y0 = (int)ceil(vmin - SGW_SLACK - 0.5);
		y1 = (int)floor(vmax + SGW_SLACK + 0.5);
	} else {
		x0 = (int)floor(umin - SGW_SLACK) - (K / 2 - 1);
		x1 = (int)floor(umax + SGW_SLACK) + K / 2;
		y0 = (int)floor(vmin - SGW_SLACK) - (K / 2 - 1);
		y1 = (int)floor(vmax + SGW_SLACK) + K / 2;
	}
	x0 = x0 < -(K - 1) ? -(K - 1) : x0;
	y0 = y0 < -(K - 1) ? -(K - 1) : y0;
	x1 = x1 > W - 1 + (K - 1) ? W - 1 + (K - 1) : x1;
	y1 = y1 > H - 1 + (K - 1) ? H - 1 + (K - 1) : y1;
	b.x0 = x0;
	b.y0 = y0;
	b.x1 = x1;
	b.y1 = y1;
	if (x1 < x0 || y1 < y0) {	/* nothing to stage */
		b.route = SGW_ROUTE_LDS;
		return b;
	}
	b.pitch = sgw_lds_pitch(x1 - x0 + 1);
	if ((int64_t)b.pitch * (y1 - y0 + 1) > lds_samples)
		return b;
	b.route = SGW_ROUTE_LDS;
	return b;
}

/* the pixel's window lies inside the staged box */
template <int K> SGW_HD bool sgw_in_box(const sgw_coord &c, const sgw_box &b) {
	return c.sx >= b.x0 && c.sx + K - 1 <= b.x1 && c.sy >= b.y0 && c.sy + K - 1 <= b.y1;
}
