/*
 * sg_ecc_plan.hpp - the host-only plan of an ECC registration call (include/sirilgpu.h,
 * sg_register_ecc_u16*), with no HIP in it, so tests/test_ecc_cpu.py builds and checks it without
 * a GPU:
 *   - the argument checks (each before any device work);
 *   - the tile grid of the prepare and iteration kernels, the source tile's halo and LDS bytes;
 *   - the per-frame scratch (blurred plane, per-workgroup partial moments, state) and the frames
 *     per chunk from a byte budget, or from the test knob SG_ECC_CHUNK (SgKnobs::ecc_chunk);
 *   - the tiles' passes themselves (sge_prep_*, sge_src_load, sge_strip; host + device: the
 *     kernels' index arithmetic and per-pixel float operations), so a host program can run the
 *     whole method tile by tile under a sanitizer.
 */
#pragma once
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include "../../include/sirilgpu.h"
#include "sg_ecc_step.h"

#define SGE_TILE_W 64		/* output tile of both kernels (columns, rows): a wave per 8-row strip */
#define SGE_TILE_H 32
#define SGE_ROWS 8		/* rows a thread walks down its column */
#define SGE_THREADS (SGE_TILE_W * (SGE_TILE_H / SGE_ROWS))
#define SGE_HALO 3		/* source tile: 1 before (gradient), 2 after (second tap + gradient) */
#define SGE_SRC_W (SGE_TILE_W + SGE_HALO)
#define SGE_SRC_H (SGE_TILE_H + SGE_HALO)
#define SGE_BLUR_R 2		/* 5x5 blur */
#define SGE_IN_W (SGE_TILE_W + 2 * SGE_BLUR_R)
#define SGE_IN_H (SGE_TILE_H + 2 * SGE_BLUR_R)
#define SGE_MIN_SIDE 8
#define SGE_MAX_SIDE 65536
#define SGE_BUDGET ((int64_t)1 << 30)	/* bytes of per-frame scratch per chunk */
#define SGE_MAX_CHUNK 65535	/* frames are the grid's z */
#define SGE_SYNC_EVERY 4	/* iteration launches between two looks at the active-frame count */

/* ------------------------------------------------------------------ prepare: clamp and blur */

/* BORDER_REFLECT_101 for the two positions past either end the blur reads; further out (the part
 * of an edge tile beyond the image, never used) the index is held inside */
SGE_HD int sge_reflect(int i, int n) {
	if (i < 0)
		i = -i;
	if (i >= n)
		i = 2 * (n - 1) - i;
	return i < 0 ? 0 : (i >= n ? n - 1 : i);
}

/* s_in[idx], idx in [0, SGE_IN_H * SGE_IN_W): convertTo(CV_8UC1) saturates */
SGE_HD uint16_t sge_prep_load(int idx, const uint16_t *img, int64_t row_pitch, int W, int H, int tx0, int ty0) {
	const int ly = idx / SGE_IN_W, lx = idx - ly * SGE_IN_W;
	const int gy = sge_reflect(ty0 - SGE_BLUR_R + ly, H), gx = sge_reflect(tx0 - SGE_BLUR_R + lx, W);
	const uint16_t v = img[(int64_t)gy * row_pitch + gx];
	return v > 255 ? 255 : v;
}

/* horizontal {1, 4, 6, 4, 1}: s_mid[idx], idx in [0, SGE_IN_H * SGE_TILE_W); at most 16 * 255 */
SGE_HD uint16_t sge_prep_h(int idx, const uint16_t *s_in) {
	const int ly = idx / SGE_TILE_W, ox = idx - ly * SGE_TILE_W;
	const uint16_t *r = s_in + ly * SGE_IN_W + ox;
	return (uint16_t)(r[0] + 4 * r[1] + 6 * r[2] + 4 * r[3] + r[4]);
}

/* vertical pass of output (ox, oy) of the tile: blurred * 256, at most 65280 */
SGE_HD uint16_t sge_prep_v(int ox, int oy, const uint16_t *s_mid) {
	const uint16_t *c = s_mid + oy * SGE_TILE_W + ox;
	return (uint16_t)((uint32_t)c[0] + 4u * c[SGE_TILE_W] + 6u * c[2 * SGE_TILE_W] + 4u * c[3 * SGE_TILE_W] +
			c[4 * SGE_TILE_W]);
}

/* ------------------------------------------------------------------ iteration: warp and moments */

struct SgeWarp {
	int iox, ioy;		/* integer source offset of the first bilinear tap */
	int mox, moy;		/* offset of the mask's nearest tap */
	float w00, w01, w10, w11;	/* (1 - fy)(1 - fx), (1 - fy) fx, fy (1 - fx), fy fx */
};

SGE_HD SgeWarp sge_warp_setup(float tx, float ty) {
	SgeWarp w;
	int fx, fy;
	sge_offsets(tx, &w.iox, &fx, &w.mox);
	sge_offsets(ty, &w.ioy, &fy, &w.moy);
	const float ax = (float)fx * (1.f / 32.f), ay = (float)fy * (1.f / 32.f);
	w.w00 = (1.f - ay) * (1.f - ax);
	w.w01 = (1.f - ay) * ax;
	w.w10 = ay * (1.f - ax);
	w.w11 = ay * ax;
	return w;
}

/* s_src[idx], idx in [0, SGE_SRC_H * SGE_SRC_W): the blurred float of source pixel
 * (sx0 + lx, sy0 + ly), 0 outside the image (border constant 0); sx0 = tile x0 + iox - 1 */
SGE_HD float sge_src_load(int idx, const uint16_t *plane, int W, int H, int sx0, int sy0) {
	const int ly = idx / SGE_SRC_W, lx = idx - ly * SGE_SRC_W;
	const int64_t gx = (int64_t)sx0 + lx, gy = (int64_t)sy0 + ly;
	if (gx < 0 || gx >= W || gy < 0 || gy >= H)
		return 0.f;
	return (float)plane[gy * W + gx] * (1.f / 256.f);
}

SGE_HD float sge_bilinear(float s00, float s01, float s10, float s11, const SgeWarp &w) {
	return s00 * w.w00 + s01 * w.w01 + s10 * w.w10 + s11 * w.w11;
}

/*
 * strip `item` in [0, SGE_THREADS): column item % SGE_TILE_W, rows (item / SGE_TILE_W) * SGE_ROWS
 * onwards of the tile at (x0, y0).  s_src rows u .. u + 3 and columns ox .. ox + 3 hold the source
 * pixels (ix - 1 .. ix + 2, iy - 1 .. iy + 2) of output row u, column ox.  The gradients of the
 * blurred source, filter2D with (-0.5, 0, 0.5) under reflect-101, are 0 in the image's first and
 * last column (gx) or row (gy) and outside it.  acc[SGE_NMOM] gains the strip's raw moments.
 */
SGE_HD void sge_strip(int item, const float *s_src, const uint16_t *tmpl, int W, int H, int x0, int y0,
		const SgeWarp &w, double *acc) {
	const int strip = item / SGE_TILE_W, ox = item - strip * SGE_TILE_W, oy0 = strip * SGE_ROWS;
	const int x = x0 + ox;
	if (x >= W || y0 + oy0 >= H)
		return;
	const int64_t sxa = (int64_t)x + w.iox, mx = (int64_t)x + w.mox;
	const bool cxa = sxa >= 1 && sxa <= W - 2, cxb = sxa + 1 >= 1 && sxa + 1 <= W - 2;
	const bool onx = mx >= 0 && mx < W;
	float R[SGE_ROWS + 3][4];
#pragma unroll
	for (int t = 0; t < SGE_ROWS + 3; t++)
#pragma unroll
		for (int c = 0; c < 4; c++)
			R[t][c] = s_src[(oy0 + t) * SGE_SRC_W + ox + c];
#pragma unroll
	for (int u = 0; u < SGE_ROWS; u++) {
		const int y = y0 + oy0 + u;
		if (y >= H)
			break;
		const int64_t sya = (int64_t)y + w.ioy, my = (int64_t)y + w.moy;
		const bool cya = sya >= 1 && sya <= H - 2, cyb = sya + 1 >= 1 && sya + 1 <= H - 2;
		const float iw = sge_bilinear(R[u + 1][1], R[u + 1][2], R[u + 2][1], R[u + 2][2], w);
		const float gx00 = cxa ? 0.5f * R[u + 1][2] - 0.5f * R[u + 1][0] : 0.f;
		const float gx01 = cxb ? 0.5f * R[u + 1][3] - 0.5f * R[u + 1][1] : 0.f;
		const float gx10 = cxa ? 0.5f * R[u + 2][2] - 0.5f * R[u + 2][0] : 0.f;
		const float gx11 = cxb ? 0.5f * R[u + 2][3] - 0.5f * R[u + 2][1] : 0.f;
		const float gy00 = cya ? 0.5f * R[u + 2][1] - 0.5f * R[u][1] : 0.f;
		const float gy01 = cya ? 0.5f * R[u + 2][2] - 0.5f * R[u][2] : 0.f;
		const float gy10 = cyb ? 0.5f * R[u + 3][1] - 0.5f * R[u + 1][1] : 0.f;
		const float gy11 = cyb ? 0.5f * R[u + 3][2] - 0.5f * R[u + 1][2] : 0.f;
		const double gx = (double)sge_bilinear(gx00, gx01, gx10, gx11, w);
		const double gy = (double)sge_bilinear(gy00, gy01, gy10, gy11, w);
		const double di = (double)iw;
		acc[SGE_HXX] += gx * gx;
		acc[SGE_HXY] += gx * gy;
		acc[SGE_HYY] += gy * gy;
		if (onx && my >= 0 && my < H) {
			const double t = (double)((float)tmpl[(int64_t)y * W + x] * (1.f / 256.f));
			acc[SGE_N] += 1.0;
			acc[SGE_SI] += di;
			acc[SGE_SII] += di * di;
			acc[SGE_ST] += t;
			acc[SGE_STT] += t * t;
			acc[SGE_STI] += t * di;
			acc[SGE_GXI] += gx * di;
			acc[SGE_GYI] += gy * di;
			acc[SGE_GXT] += gx * t;
			acc[SGE_GYT] += gy * t;
			acc[SGE_GX] += gx;
			acc[SGE_GY] += gy;
		} else {
			acc[SGE_OGXI] += gx * di;
			acc[SGE_OGYI] += gy * di;
		}
	}
}

/* ------------------------------------------------------------------ the plan */

struct SgEccPlan {
	int W = 0, H = 0, nframes = 0, ref_image = 0;
	int64_t frame_pitch = 0, row_pitch = 0;
	int tiles_x = 0, tiles_y = 0, tiles = 0, halo = SGE_HALO;
	int src_w = SGE_SRC_W, src_h = SGE_SRC_H;
	size_t lds_iter = 0, lds_prep = 0;
	size_t plane_bytes = 0, partial_bytes = 0, state_bytes = 0, frame_bytes = 0;	/* per frame */
	int chunk = 0, nchunks = 0;
	char err[256] = "";
};

static inline int sge_fail(SgEccPlan &p, int code, const char *msg) {
	snprintf(p.err, sizeof p.err, "%s", msg);
	return code;
}

/* frame_pitch / row_pitch in elements, 0 = tight (row_pitch W, frame_pitch H * row_pitch); budget
 * <= 0 = SGE_BUDGET; force_chunk > 0 = that many frames per chunk whatever the budget */
static inline int sg_ecc_plan(int W, int H, int nframes, int ref_image, int64_t frame_pitch, int64_t row_pitch,
		int64_t budget, int force_chunk, SgEccPlan &p) {
	p = SgEccPlan();
	if (W < SGE_MIN_SIDE || H < SGE_MIN_SIDE)
		return sge_fail(p, SG_ERR_SIZE, "ecc: width or height below 8 (the 5x5 blur and the gradients need the room)");
	if (W > SGE_MAX_SIDE || H > SGE_MAX_SIDE || (int64_t)W * H >= ((int64_t)1 << 31))
		return sge_fail(p, SG_ERR_SIZE, "ecc: a side above 65536 or a plane of 2^31 pixels or more");
	if (nframes < 1)
		return sge_fail(p, SG_ERR_SIZE, "ecc: no frames");
	if (ref_image < 0 || ref_image >= nframes)
		return sge_fail(p, SG_ERR_SIZE, "ecc: ref_image outside [0, nframes)");
	if (row_pitch == 0)
		row_pitch = W;
	if (frame_pitch == 0)
		frame_pitch = (int64_t)H * row_pitch;
	if (row_pitch < W)
		return sge_fail(p, SG_ERR_SIZE, "ecc: row_pitch below the width");
	if (frame_pitch < (int64_t)(H - 1) * row_pitch + W)
		return sge_fail(p, SG_ERR_SIZE, "ecc: frame_pitch below one frame's extent");
	p.W = W;
	p.H = H;
	p.nframes = nframes;
	p.ref_image = ref_image;
	p.frame_pitch = frame_pitch;
	p.row_pitch = row_pitch;
	p.tiles_x = (W + SGE_TILE_W - 1) / SGE_TILE_W;
	p.tiles_y = (H + SGE_TILE_H - 1) / SGE_TILE_H;
	p.tiles = p.tiles_x * p.tiles_y;
	p.lds_iter = (size_t)SGE_SRC_W * SGE_SRC_H * sizeof(float);
	p.lds_prep = ((size_t)SGE_IN_W * SGE_IN_H + (size_t)SGE_TILE_W * SGE_IN_H) * sizeof(uint16_t);
	p.plane_bytes = (size_t)W * H * sizeof(uint16_t);
	p.partial_bytes = (size_t)p.tiles * SGE_NMOM * sizeof(double);
	p.state_bytes = sizeof(sge_state) + sizeof(uint32_t);	/* the state and the frame's ticket */
	p.frame_bytes = p.plane_bytes + p.partial_bytes + p.state_bytes;
	int64_t c = (budget > 0 ? budget : SGE_BUDGET) / (int64_t)p.frame_bytes;
	if (force_chunk > 0)
		c = force_chunk;
	if (c < 1)
		c = 1;
	if (c > SGE_MAX_CHUNK)
		c = SGE_MAX_CHUNK;
	if (c > nframes)
		c = nframes;
	p.chunk = (int)c;
	p.nchunks = (nframes + p.chunk - 1) / p.chunk;
	return SG_OK;
}
