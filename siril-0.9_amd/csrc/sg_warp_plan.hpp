/*
 * sg_warp_plan.hpp - the host-only plan of a sequence warp call (include/sirilgpu.h,
 * sg_warp_frames_u16*), with no HIP in it, so tests/test_warp_plan_cpu.py builds it without a GPU:
 *   - the argument checks (each before any device work);
 *   - the inverse matrices (cv::invert's closed form, as sg_warp.hip's sg_invert3; a singular
 *     homography leaves a zero matrix);
 *   - OpenCV's block width bw, the tap count K, the tile grid (SGW_TILE_X x SGW_TILE_Y destination
 *     pixels per workgroup, sg_warp_tile.h) and the workgroup's LDS;
 *   - the default route per interpolation, from the measurement (DESIGN.md §2 "Sequence warp"): a
 *     tile's taps come from LDS for linear and Lanczos-4, from global memory for nearest (one tap:
 *     nothing to share) and cubic (the A/B lost); SG_WARP_ROUTE 1 sends every tile to global
 *     memory, 2 every tile whose box fits to LDS;
 *   - the frames per launch: frame x layer is the grid's z dimension, at most 65535;
 *   - the per-frame table that goes to the device and the scratch that holds it.
 *
 * Device scratch, bytes: [0, 16384) the counters in SGW_CTR_SHARDS shards of 64 bytes (tiles_lds,
 * tiles_gather, pixels_stray: u64 each, then a pad; a workgroup adds to the shard its grid index
 * picks, the host sums them), then nframes entries of SGW_ENTRY_BYTES = 80: M (9 doubles, row-major), action (int32),
 * slot (int32).  Entry f describes source frame f of the call.
 */
#pragma once
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <algorithm>
#include <vector>
#include "../../include/sirilgpu.h"
#include "sg_warp_tile.h"

#define SGW_ENTRY_BYTES 80
#define SGW_CTR_SHARDS 256
#define SGW_CTR_STRIDE 8	/* u64 per shard: a 64-byte line of its own */
#define SGW_CTR_BYTES (SGW_CTR_SHARDS * SGW_CTR_STRIDE * 8)
#define SGW_MAX_GRID_Z 65535

struct SgWarpEntry {
	double M[9];
	int32_t action, slot;
};
static_assert(sizeof(SgWarpEntry) == SGW_ENTRY_BYTES, "per-frame table layout");

struct SgWarpPlan {
	int W = 0, H = 0, C = 0, oW = 0, oH = 0;
	int interp = 0, K = 0, bw = 0;
	int64_t frame_pitch = 0, out_frame_pitch = 0;
	int nframes = 0, napply = 0, ncopy = 0, max_slot = -1;
	int tiles_x = 0, tiles_y = 0;
	int64_t tiles = 0;		/* of one layer of one frame */
	int lds_default = 0;		/* the interpolation's measured default is the LDS route */
	int force_gather = 0;		/* every tile reads global memory */
	int lds_samples = 0;
	size_t lds_bytes = 0;		/* the staged box; the workgroup also keeps its sgw_box */
	int frames_per_launch = 0, nlaunches = 0;
	size_t table_offset = 0, table_bytes = 0, work_bytes = 0;
	char err[256] = "";
};

static inline int sgw_fail(SgWarpPlan &p, int code, const char *msg) {
	snprintf(p.err, sizeof p.err, "%s", msg);
	return code;
}

/* cv::invert(DECOMP_LU) of a 3x3: closed form with 1/det; a zero matrix if singular */
static inline int sgw_invert3(const double *a, double *o) {
	const double d = a[0] * (a[4] * a[8] - a[5] * a[7]) - a[1] * (a[3] * a[8] - a[5] * a[6]) +
		a[2] * (a[3] * a[7] - a[4] * a[6]);
	if (d == 0.0) {
		for (int i = 0; i < 9; i++)
			o[i] = 0.0;
		return 0;
	}
	const double t = 1.0 / d;
	o[0] = (a[4] * a[8] - a[5] * a[7]) * t;
	o[1] = (a[2] * a[7] - a[1] * a[8]) * t;
	o[2] = (a[1] * a[5] - a[2] * a[4]) * t;
	o[3] = (a[5] * a[6] - a[3] * a[8]) * t;
	o[4] = (a[0] * a[8] - a[2] * a[6]) * t;
	o[5] = (a[2] * a[3] - a[0] * a[5]) * t;
	o[6] = (a[3] * a[7] - a[4] * a[6]) * t;
	o[7] = (a[1] * a[6] - a[0] * a[7]) * t;
	o[8] = (a[0] * a[4] - a[1] * a[3]) * t;
	return 1;
}

#define SGW_KNOB_PLAN 0
#define SGW_KNOB_GATHER 1
#define SGW_KNOB_LDS 2

/* in / out: the addresses of the two sequences (device or host; the byte ranges they span must not
 * overlap); action == NULL: every frame APPLY; out_slot == NULL: frame f to slot f; route_knob:
 * SG_WARP_ROUTE.  table gets one entry per frame. */
static inline int sg_warp_plan(const sg_warp_seq_desc *d, int nframes, const double *hom, const int *action, const int *out_slot,
		const void *in, const void *out, int route_knob, SgWarpPlan &p, std::vector<SgWarpEntry> &table) {
	p = SgWarpPlan();
	table.clear();
	if (!d)
		return sgw_fail(p, SG_ERR_GENERIC, "warp: missing descriptor");
	if (d->width <= 0 || d->height <= 0 || d->out_width <= 0 || d->out_height <= 0)
		return sgw_fail(p, SG_ERR_SIZE, "warp: width or height not positive");
	if ((int64_t)d->width * d->height >= ((int64_t)1 << 31) || (int64_t)d->out_width * d->out_height >= ((int64_t)1 << 31))
		return sgw_fail(p, SG_ERR_SIZE, "warp: a plane of 2^31 pixels or more");
	if (d->nb_layers < 1 || d->nb_layers > 3)
		return sgw_fail(p, SG_ERR_SIZE, "warp: nb_layers outside 1..3");
	if (d->interpolation < 0 || d->interpolation > 4)
		return sgw_fail(p, SG_ERR_GENERIC, "warp: interpolation outside 0..4");
	if (nframes < 1)
		return sgw_fail(p, SG_ERR_SIZE, "warp: no frames");
	const int64_t in_elems = (int64_t)d->width * d->height * d->nb_layers, out_elems = (int64_t)d->out_width * d->out_height * d->nb_layers;
	const int64_t fp = d->frame_pitch ? d->frame_pitch : in_elems, op = d->out_frame_pitch ? d->out_frame_pitch : out_elems;
	if (fp < in_elems)
		return sgw_fail(p, SG_ERR_SIZE, "warp: frame_pitch below one frame");
	if (op < out_elems)
		return sgw_fail(p, SG_ERR_SIZE, "warp: out_frame_pitch below one frame");
	if (!hom || !in || !out)
		return sgw_fail(p, SG_ERR_GENERIC, "warp: missing frames, homographies or output");
	p.W = d->width;
	p.H = d->height;
	p.C = d->nb_layers;
	p.oW = d->out_width;
	p.oH = d->out_height;
	p.interp = d->interpolation == 2 ? 1 : d->interpolation;	/* INTER_AREA is INTER_LINEAR in warpPerspective */
	p.K = sgw_ksize(p.interp);
	p.bw = sgw_block_width(p.oW, p.oH);
	p.frame_pitch = fp;
	p.out_frame_pitch = op;
	p.nframes = nframes;
	p.tiles_x = (p.oW + SGW_TILE_X - 1) / SGW_TILE_X;
	p.tiles_y = (p.oH + SGW_TILE_Y - 1) / SGW_TILE_Y;
	if (p.tiles_y > SGW_MAX_GRID_Z)
		return sgw_fail(p, SG_ERR_SIZE, "warp: out_height above 16 x 65535");
	p.tiles = (int64_t)p.tiles_x * p.tiles_y;
	std::vector<int> slots;
	table.resize((size_t)nframes);
	for (int f = 0; f < nframes; f++) {
		SgWarpEntry &e = table[(size_t)f];
		e.action = action ? action[f] : SG_WARP_APPLY;
		e.slot = out_slot ? out_slot[f] : f;
		sgw_invert3(hom + (size_t)f * 9, e.M);
		if (e.action == SG_WARP_SKIP)
			continue;
		if (e.action != SG_WARP_APPLY && e.action != SG_WARP_COPY)
			return sgw_fail(p, SG_ERR_GENERIC, "warp: an action that is not SKIP, APPLY or COPY");
		if (e.action == SG_WARP_COPY && (p.W != p.oW || p.H != p.oH))
			return sgw_fail(p, SG_ERR_GENERIC, "warp: COPY needs equal source and output sizes");
		if (e.slot < 0)
			return sgw_fail(p, SG_ERR_GENERIC, "warp: a written frame with a slot below 0");
		slots.push_back(e.slot);
		p.napply += e.action == SG_WARP_APPLY;
		p.ncopy += e.action == SG_WARP_COPY;
		p.max_slot = std::max(p.max_slot, e.slot);
	}
	std::sort(slots.begin(), slots.end());
	if (std::adjacent_find(slots.begin(), slots.end()) != slots.end())
		return sgw_fail(p, SG_ERR_GENERIC, "warp: two written frames with the same slot");
	if (p.max_slot >= 0) {
		const uintptr_t a0 = (uintptr_t)in, a1 = a0 + (size_t)((nframes - 1) * fp + in_elems) * sizeof(uint16_t);
		const uintptr_t b0 = (uintptr_t)out, b1 = b0 + (size_t)(p.max_slot * op + out_elems) * sizeof(uint16_t);
		if (a0 < b1 && b0 < a1)
			return sgw_fail(p, SG_ERR_GENERIC, "warp: the source and output sequences overlap");
	}
	p.lds_default = p.K == 2 || p.K == 8;
	p.force_gather = route_knob == SGW_KNOB_GATHER || (route_knob != SGW_KNOB_LDS && !p.lds_default);
	p.lds_samples = SGW_LDS_SAMPLES;
	p.lds_bytes = (size_t)p.lds_samples * sizeof(uint16_t);
	p.frames_per_launch = std::min(nframes, SGW_MAX_GRID_Z / p.C);
	p.nlaunches = (nframes + p.frames_per_launch - 1) / p.frames_per_launch;
	p.table_offset = SGW_CTR_BYTES;
	p.table_bytes = (size_t)nframes * SGW_ENTRY_BYTES;
	p.work_bytes = p.table_offset + p.table_bytes;
	return SG_OK;
}
