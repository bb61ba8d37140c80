/*
 * sg_seqpsf_plan.hpp - the host-only plan of a one-star registration call (include/sirilgpu.h,
 * sg_seqpsf_u16*), with no HIP in it, so tests/test_seqpsf_plan_cpu.py builds and checks it without
 * a GPU:
 *   - the argument checks (each before any device work);
 *   - the per-frame table of the kernels: whether a frame runs and, for the parallel framings, its
 *     clamped area (step 1 of the contract);
 *   - the LDS bytes of a workgroup and the grid.
 */
#pragma once
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <vector>
#include "sg_host_batch.hpp"
#include "sg_seqpsf.h"

/* threads of a workgroup, one compile-time constant for both kernels, so that a chain on a star that
 * does not move gives ORIGINAL framing's bits (the sums' order depends on it).  A/B: make
 * EXTRA=-DSGQ_THREADS=n, n = 64, 256 or 1024; DESIGN.md §2 "One-star registration" has the measurement
 * behind the default (profiles/seqpsf_4096x480x640.log). */
#ifndef SGQ_THREADS
#define SGQ_THREADS 256
#endif
#define SGQ_NSUM 36		/* the sums of a p = 7 evaluation: 28 + 7 + 1 */
#define SGQ_HIST 256		/* bins of one radix-select pass */
#define SGQ_MIN_SIDE 8		/* W, H: the limits of sg_register_ecc_u16_device */
#define SGQ_MAX_SIDE 65536

/* one frame of the per-frame table */
struct SgSeqpsfItem {
	int32_t run;		/* 0 = excluded */
	int32_t x, y;		/* the clamped area (parallel framings) */
	int32_t pad;
};

struct SgSeqpsfPlan {
	int W = 0, H = 0, nframes = 0, framing = 0, w = 0, h = 0, fit_angle = 0;
	int64_t frame_pitch = 0, row_pitch = 0;
	double norm = 0., scale_x = 0., scale_y = 0.;
	int start_x = 0, start_y = 0;		/* FOLLOW_STAR: the chain's starting (unclamped) area */
	size_t lds_box = 0, lds_bytes = 0;	/* the box as u16, 16-byte aligned; all of a workgroup's LDS */
	unsigned grid = 0, threads = 0;
	size_t table_bytes = 0, record_bytes = 0, work_bytes = 0;	/* the table, the records (+ the carry), both */
	std::vector<SgSeqpsfItem> items;
	char err[256] = "";
};

static inline int sgq_fail(SgSeqpsfPlan &p, int code, const char *msg) {
	snprintf(p.err, sizeof p.err, "%s", msg);
	return code;
}

/* LDS of a workgroup: the box, the wave partials of one evaluation, the radix-select bins, and 16
 * 8-byte words of scalars (the max keys of the waves, the selected bin, the carried area) */
static inline size_t sgq_lds_bytes(int w, int h, int threads) {
	const size_t waves = (size_t)threads / 64;
	return sg_up16((size_t)w * h * sizeof(uint16_t)) + waves * SGQ_NSUM * sizeof(double) +
			(size_t)SGQ_HIST * sizeof(uint32_t) + 16 * sizeof(uint64_t) + waves * sizeof(uint64_t);
}

/* frame_pitch / row_pitch in elements, 0 = tight; carry: the chain's start when FOLLOW_STAR, or NULL */
static inline int sg_seqpsf_plan(const sg_seqpsf_desc *d, int W, int H, int nframes, int64_t frame_pitch, int64_t row_pitch,
		const int *included, const int *reg_shiftx, const int *reg_shifty, const sg_rect *carry, SgSeqpsfPlan &p) {
	p = SgSeqpsfPlan();
	if (!d)
		return sgq_fail(p, SG_ERR_GENERIC, "seqpsf: missing descriptor");
	if (W < SGQ_MIN_SIDE || H < SGQ_MIN_SIDE)
		return sgq_fail(p, SG_ERR_SIZE, "seqpsf: width or height below 8");
	if (W > SGQ_MAX_SIDE || H > SGQ_MAX_SIDE || (int64_t)W * H >= ((int64_t)1 << 31))
		return sgq_fail(p, SG_ERR_SIZE, "seqpsf: a side above 65536 or a plane of 2^31 pixels or more");
	if (nframes < 1)
		return sgq_fail(p, SG_ERR_SIZE, "seqpsf: no frames");
	if (row_pitch == 0)
		row_pitch = W;
	if (frame_pitch == 0)
		frame_pitch = (int64_t)H * row_pitch;
	if (row_pitch < W)
		return sgq_fail(p, SG_ERR_SIZE, "seqpsf: row_pitch below the width");
	if (frame_pitch < (int64_t)(H - 1) * row_pitch + W)
		return sgq_fail(p, SG_ERR_SIZE, "seqpsf: frame_pitch below one frame's extent");
	const int w = d->area.w, h = d->area.h;
	if (w < 1 || h < 1)
		return sgq_fail(p, SG_ERR_SIZE, "seqpsf: the area's width or height below 1 (select an area first)");
	if (w > SG_SEQPSF_MAX_SIDE || h > SG_SEQPSF_MAX_SIDE)
		return sgq_fail(p, SG_ERR_SIZE, "seqpsf: the area's width or height above 128");
	if (w > W || h > H)
		return sgq_fail(p, SG_ERR_SIZE, "seqpsf: the area is larger than the image");
	if (d->framing != SG_SEQPSF_ORIGINAL && d->framing != SG_SEQPSF_REGISTERED && d->framing != SG_SEQPSF_FOLLOW_STAR)
		return sgq_fail(p, SG_ERR_GENERIC, "seqpsf: unknown framing");
	if (d->framing == SG_SEQPSF_REGISTERED && (!reg_shiftx || !reg_shifty))
		return sgq_fail(p, SG_ERR_GENERIC, "seqpsf: REGISTERED framing without the frames' shifts");
	if (d->norm != 65535.0)
		return sgq_fail(p, SG_ERR_GENERIC, "seqpsf: norm must be 65535 (8-bit statistics are not implemented)");
	if (!isfinite(d->fwhm_scale_x) || !isfinite(d->fwhm_scale_y))
		return sgq_fail(p, SG_ERR_GENERIC, "seqpsf: a FWHM scale is not finite");
	p.W = W;
	p.H = H;
	p.nframes = nframes;
	p.framing = d->framing;
	p.w = w;
	p.h = h;
	p.fit_angle = d->fit_angle != 0;
	p.frame_pitch = frame_pitch;
	p.row_pitch = row_pitch;
	p.norm = d->norm;
	p.scale_x = d->fwhm_scale_x;
	p.scale_y = d->fwhm_scale_y;
	const bool chain = d->framing == SG_SEQPSF_FOLLOW_STAR;
	p.start_x = chain && carry ? carry->x : d->area.x;
	p.start_y = chain && carry ? carry->y : d->area.y;
	p.items.resize((size_t)nframes);
	for (int f = 0; f < nframes; f++) {
		SgSeqpsfItem &it = p.items[(size_t)f];
		it.run = !included || included[f];
		it.pad = 0;
		it.x = p.start_x;
		it.y = p.start_y;
		if (!chain)
			sq_frame_area(d->framing == SG_SEQPSF_REGISTERED, d->area.x, d->area.y, reg_shiftx ? reg_shiftx[f] : 0,
					reg_shifty ? reg_shifty[f] : 0, W, H, w, h, &it.x, &it.y);
	}
	p.lds_box = sg_up16((size_t)w * h * sizeof(uint16_t));
	p.threads = SGQ_THREADS;
	p.lds_bytes = sgq_lds_bytes(w, h, (int)p.threads);
	p.grid = chain ? 1u : (unsigned)nframes;
	p.table_bytes = sg_up16((size_t)nframes * sizeof(SgSeqpsfItem));
	p.record_bytes = sg_up16((size_t)nframes * sizeof(sg_seqpsf_frame)) + 16;
	p.work_bytes = p.table_bytes + p.record_bytes;
	return SG_OK;
}
