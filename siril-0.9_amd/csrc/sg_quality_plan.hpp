/*
 * sg_quality_plan.hpp - the host-only plan of a quality estimate call (include/sirilgpu.h,
 * sg_quality_u16*), with no HIP in it, so tests/test_quality_plan_cpu.py and the stand-alone
 * program of tests/test_quality_cpu.py build it without a GPU:
 *   - the argument checks (each before any device work);
 *   - the route: none (xs < 2 || ys < 2: every result is 0.0), resident (a frame's samples and
 *     smoothed plane in one workgroup's LDS) or tiled (a u16 scratch plane in HBM);
 *   - the resident route's LDS layout and the largest plane it takes;
 *   - the tiled route's tile grid and LDS bytes (the tiles' index functions are sg_quality.h's);
 *   - the scratch of a chunk and the frames per chunk from a byte budget or from SG_QUALITY_CHUNK;
 *   - the two bookkeeping helpers sg_quality_normalize and sg_quality_select.
 *
 * Resident LDS, bytes: [0, P) the samples (u16, stretched in place), [P, 2P) the smoothed plane
 * (u16), P = xs * ys * 2 rounded up to 16; then 32 bytes: the maximum (u32), a pad, val (u64),
 * pixels (u64).  2P + 32 must not exceed the budget (SGQ_LDS_MAX = 160 KiB, or SG_QUALITY_LDS).
 *
 * Scratch of a chunk of n frames: the frame list (int32 each) and the results (double each), both
 * rounded up to 16; for the tiled route also n sample planes of P bytes and n accumulators of 32
 * bytes (max u32, pad, val u64, pixels u64), cleared per chunk.
 */
#pragma once
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <algorithm>
#include <vector>
#include "../../include/sirilgpu.h"
#include "sg_quality.h"
#include "sg_host_batch.hpp"

#define SGQ_ROUTE_NONE 0
#define SGQ_ROUTE_RESIDENT 1
#define SGQ_ROUTE_TILED 2
#define SGQ_LDS_MAX (160 * 1024)	/* a gfx950 workgroup's LDS */
#define SGQ_LDS_TAIL 32
#define SGQ_RES_THREADS 1024
#define SGQ_THREADS 256		/* of both tiled passes: SGQ_TILE_X x SGQ_TILE_Y samples (sg_quality.h) per workgroup */
#define SGQ_ACC_BYTES 32
#define SGQ_BUDGET ((int64_t)1 << 28)
#define SGQ_MAX_CHUNK 65535	/* a chunk's frames are a grid dimension */

struct SgQualityPlan {
	int W = 0, H = 0, nframes = 0, nwork = 0;
	int64_t frame_pitch = 0, row_pitch = 0;
	sgq_geom g = {0, 0, 0, 0};
	int64_t nsamples = 0;
	int route = SGQ_ROUTE_NONE;
	int lds_budget = 0, resident_fits = 0;
	size_t plane_bytes = 0;		/* P */
	size_t lds_bytes = 0;		/* 2P + 32, whatever the route */
	int64_t resident_max_samples = 0;	/* the largest xs * ys the budget takes */
	int tiles_x = 0, tiles_y = 0;
	size_t lds_tile = 0;		/* the gradient pass's two tiles */
	int chunk = 0, nchunks = 0;
	size_t list_bytes = 0, out_bytes = 0, planes_bytes = 0, acc_bytes = 0, total_bytes = 0;	/* of a full chunk */
	char err[256] = "";
};

static inline int sgq_fail(SgQualityPlan &p, int code, const char *msg) {
	snprintf(p.err, sizeof p.err, "%s", msg);
	return code;
}

static inline size_t sgq_chunk_bytes(SgQualityPlan &p, int64_t chunk) {
	p.list_bytes = sg_up16((size_t)chunk * sizeof(int32_t));
	p.out_bytes = sg_up16((size_t)chunk * sizeof(double));
	p.planes_bytes = p.route == SGQ_ROUTE_TILED ? (size_t)chunk * p.plane_bytes : 0;
	p.acc_bytes = p.route == SGQ_ROUTE_TILED ? (size_t)chunk * SGQ_ACC_BYTES : 0;
	p.total_bytes = p.list_bytes + p.out_bytes + p.planes_bytes + p.acc_bytes;
	return p.total_bytes;
}

/* frame_pitch / row_pitch in elements, 0 = tight; nwork = the frames the call estimates (the
 * included ones; < 0 = nframes); budget <= 0 = SGQ_BUDGET; force_route: SG_QUALITY_ROUTE (0 the
 * plan's choice, 1 resident where it fits, 2 tiled); force_chunk > 0 = SG_QUALITY_CHUNK;
 * lds_budget <= 0 = SGQ_LDS_MAX (SG_QUALITY_LDS) */
static inline int sg_quality_plan(int W, int H, int nframes, int nwork, int64_t frame_pitch, int64_t row_pitch,
		int64_t budget, int force_route, int force_chunk, int lds_budget, SgQualityPlan &p) {
	p = SgQualityPlan();
	if (W <= 0 || H <= 0)
		return sgq_fail(p, SG_ERR_SIZE, "quality: width or height not positive");
	if ((int64_t)W * H >= ((int64_t)1 << 31))
		return sgq_fail(p, SG_ERR_SIZE, "quality: a plane of 2^31 pixels or more");
	if (nframes < 1)
		return sgq_fail(p, SG_ERR_SIZE, "quality: no frames");
	if (row_pitch == 0)
		row_pitch = W;
	if (frame_pitch == 0)
		frame_pitch = (int64_t)H * row_pitch;
	if (row_pitch < W)
		return sgq_fail(p, SG_ERR_SIZE, "quality: row_pitch below the width");
	if (frame_pitch < (int64_t)(H - 1) * row_pitch + W)
		return sgq_fail(p, SG_ERR_SIZE, "quality: frame_pitch below one frame's extent");
	p.W = W;
	p.H = H;
	p.nframes = nframes;
	p.nwork = nwork < 0 || nwork > nframes ? nframes : nwork;
	p.frame_pitch = frame_pitch;
	p.row_pitch = row_pitch;
	p.g = sgq_geometry(W, H);
	p.lds_budget = lds_budget <= 0 || lds_budget > SGQ_LDS_MAX ? SGQ_LDS_MAX : lds_budget;
	p.resident_max_samples = p.lds_budget < SGQ_LDS_TAIL + 32 ? 0 : (int64_t)(((p.lds_budget - SGQ_LDS_TAIL) / 2) & ~15) / 2;
	if (p.g.xs < 2 || p.g.ys < 2)
		return SG_OK;	/* route none: 0.0 for every frame, nothing launched */
	p.nsamples = (int64_t)p.g.xs * p.g.ys;
	p.plane_bytes = sg_up16((size_t)p.nsamples * sizeof(uint16_t));
	p.lds_bytes = 2 * p.plane_bytes + SGQ_LDS_TAIL;
	p.resident_fits = p.nsamples <= p.resident_max_samples;
	p.route = force_route != SGQ_ROUTE_TILED && p.resident_fits ? SGQ_ROUTE_RESIDENT : SGQ_ROUTE_TILED;
	p.tiles_x = (p.g.xs + SGQ_TILE_X - 1) / SGQ_TILE_X;
	p.tiles_y = (p.g.ys + SGQ_TILE_Y - 1) / SGQ_TILE_Y;
	p.lds_tile = (size_t)(SGQ_ST_W * SGQ_ST_H + SGQ_SM_W * SGQ_SM_H) * sizeof(uint16_t);
	if (p.nwork == 0)
		return SG_OK;
	int64_t c = (budget > 0 ? budget : SGQ_BUDGET) / (int64_t)sgq_chunk_bytes(p, 1);
	if (force_chunk > 0)
		c = force_chunk;
	c = std::max<int64_t>(1, std::min<int64_t>(c, std::min<int64_t>(p.nwork, SGQ_MAX_CHUNK)));
	sgq_chunk_bytes(p, c);
	p.chunk = (int)c;
	p.nchunks = (p.nwork + p.chunk - 1) / p.chunk;
	return SG_OK;
}

static inline int sgq_msg(char *msg, int msg_len, int code, const char *text) {
	if (msg && msg_len > 0)
		snprintf(msg, (size_t)msg_len, "%s", text);
	return code;
}

/* the bookkeeping of register_ecc (registration.c:838, 899-905) and normalizeQualityData
 * (:163-176), in the serial frame order; see include/sirilgpu.h */
static inline int sgq_normalize(int nframes, int ref_image, const double *raw, const int *measured, const int *normalized,
		double *quality, double *q_min_out, double *q_max_out, int *q_index_out, char *msg, int msg_len) {
	if (nframes < 1 || ref_image < 0 || ref_image >= nframes)
		return sgq_msg(msg, msg_len, SG_ERR_SIZE, "quality: no frames, or ref_image outside [0, nframes)");
	if (!raw || !quality)
		return sgq_msg(msg, msg_len, SG_ERR_GENERIC, "quality: missing raw or output array");
	double q_min, q_max;
	q_min = q_max = raw[ref_image];
	int q_index = ref_image;
	for (int frame = 0; frame < nframes; frame++) {
		if (frame == ref_image) {
			quality[frame] = raw[frame];
			continue;
		}
		if (measured && !measured[frame]) {
			quality[frame] = 0.0;	/* the regdata is calloc'ed and the frame never measured */
			continue;
		}
		const double qual = raw[frame];
		quality[frame] = qual;
		if (qual > q_max) {
			q_max = qual;
			q_index = frame;
		}
		q_min = q_min < qual ? q_min : qual;	/* the min() macro of core/siril.h */
	}
	for (int frame = 0; frame < nframes; frame++) {
		if (normalized && !normalized[frame])
			continue;
		quality[frame] -= q_min;
		quality[frame] /= (q_max - q_min);
	}
	if (q_min_out)
		*q_min_out = q_min;
	if (q_max_out)
		*q_max_out = q_max;
	if (q_index_out)
		*q_index_out = q_index;
	if (msg && msg_len > 0)
		msg[0] = 0;
	return SG_OK;
}

/* compute_highest_accepted_quality (stacking.c:2283-2310), stack_filter_quality (:2204-2213)
 * and fill_list_of_unfiltered_images (:2230-2241); see include/sirilgpu.h */
static inline int sgq_select(int nframes, const double *quality, const int *included, double percent, double *threshold,
		int *selected, int *nselected, char *msg, int msg_len) {
	if (nframes < 1)
		return sgq_msg(msg, msg_len, SG_ERR_SIZE, "quality: no frames");
	if (!quality || !threshold || !nselected)
		return sgq_msg(msg, msg_len, SG_ERR_GENERIC, "quality: missing quality, threshold or count");
	if (msg && msg_len > 0)
		msg[0] = 0;
	for (int i = 0; i < nframes; i++)
		if ((!included || included[i]) && quality[i] < 0.0) {
			*threshold = 0.0;
			*nselected = 0;
			return SG_OK;
		}
	for (int i = 0; i < nframes; i++)
		if (quality[i] != quality[i])
			return sgq_msg(msg, msg_len, SG_ERR_GENERIC, "quality: a NaN among the values (the reference's sort is undefined)");
	const double at = (100.0 - percent) * (double)nframes / 100.0;
	if (!(at > -1.0 && at < (double)nframes))
		return sgq_msg(msg, msg_len, SG_ERR_GENERIC, "quality: the percentage indexes outside the sorted values (the reference reads past its array)");
	std::vector<double> val(quality, quality + nframes);
	std::sort(val.begin(), val.end());
	const double thr = val[(int)at];
	int n = 0;
	for (int i = 0; i < nframes; i++)
		if ((!included || included[i]) && quality[i] > 0.0 && quality[i] >= thr) {
			if (selected)
				selected[n] = i;
			n++;
		}
	*threshold = thr;
	*nselected = n;
	return SG_OK;
}
