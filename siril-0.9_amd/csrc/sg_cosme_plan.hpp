/*
 * sg_cosme_plan.hpp - the host-only plan of an automatic cosmetic correction call
 * (include/sirilgpu.h, sg_cosme_autodetect*), with no HIP in it, so tests/test_cosme_plan_cpu.py
 * builds and checks it without a GPU:
 *   - the argument checks (each before any device work);
 *   - the tile grid of the main pass, its halo (2 plain, 4 CFA) and LDS bytes;
 *   - the scratch of one chunk of frames and the frames per chunk from a byte budget, or from the
 *     test knob SG_COSME_CHUNK (SgKnobs::cosme_chunk); the list capacity, or SG_COSME_LIST.
 * Scratch of a chunk, all indexed by the chunk's pixel id = (frame * C + layer) * W * H + pixel,
 * which must fit 32 bits:
 *   state   u16 per pixel: the corrected value of a pixel whose kind bit is set (written sparsely,
 *           never cleared: memory, not traffic);
 *   4 bit planes (hot, cold, active of the even and of the odd rounds), cleared per chunk;
 *   2 lists of pixel ids (the active pixels of a round), list_cap entries each; a round whose
 *           count exceeds the capacity walks its active plane instead;
 *   the 65536-bin histograms, the rules and the counters.
 */
#pragma once
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include "../../include/sirilgpu.h"
#include "sg_cosme.h"
#include "sg_host_batch.hpp"

#define SGC_MAX_LAYERS 3
#define SGC_BINS 65536
#define SGC_HIST_CHUNK 65535	/* samples per histogram workgroup: its u16 LDS counters cannot wrap */
#define SGC_BUDGET ((int64_t)1 << 30)
#define SGC_MAX_Z 65535		/* frame * C + layer is the main pass's grid z */
#define SGC_GROUP 4		/* rounds launched between two looks at the active count; even */
#define SGC_ROUND_BLOCKS 1024	/* workgroups of a round (grid-stride over its list or plane) */
#define SGC_MIN_LIST ((int64_t)1 << 16)
#define SGC_NCOUNT (SGC_GROUP + 1)	/* active counts of a group of rounds */

struct SgCosmePlan {
	int W = 0, H = 0, C = 0, nframes = 0, is_cfa = 0, step = 1, halo = 2;
	double sig0 = 0., sig1 = 0., amount = 0.;
	int64_t npix = 0, frame_stride = 0;
	int tiles_x = 0, tiles_y = 0, in_w = 0, in_h = 0;
	size_t lds_tile = 0;
	int hist_blocks = 0;		/* per layer */
	int chunk = 0, nchunks = 0;
	/* of a full chunk */
	uint64_t chunk_pixels = 0, plane_words = 0;
	size_t state_bytes = 0, plane_bytes = 0, list_bytes = 0, hist_bytes = 0, rule_bytes = 0, count_bytes = 0;
	size_t total_bytes = 0;
	uint32_t list_cap = 0;
	char err[256] = "";
};

static inline int sgc_fail(SgCosmePlan &p, int code, const char *msg) {
	snprintf(p.err, sizeof p.err, "%s", msg);
	return code;
}

/* the scratch of `chunk` frames; 0 when their pixel ids do not fit 32 bits */
static inline size_t sgc_chunk_bytes(SgCosmePlan &p, int64_t chunk, int force_list = 0) {
	const uint64_t px = (uint64_t)chunk * (uint64_t)p.C * (uint64_t)p.npix;
	if (px > 0xFFFFFFFFull - 64)
		return 0;
	p.chunk_pixels = px;
	p.plane_words = (px + 31) / 32;
	p.state_bytes = sg_up16((size_t)px * sizeof(uint16_t));
	p.plane_bytes = sg_up16((size_t)p.plane_words * sizeof(uint32_t));
	int64_t cap = (int64_t)(px / 8);
	if (cap < SGC_MIN_LIST)
		cap = SGC_MIN_LIST;
	if (force_list > 0)
		cap = force_list;
	p.list_cap = (uint32_t)cap;
	p.list_bytes = sg_up16((size_t)cap * sizeof(uint32_t));
	p.hist_bytes = (size_t)chunk * p.C * SGC_BINS * sizeof(uint32_t);
	p.rule_bytes = sg_up16((size_t)chunk * p.C * sizeof(sgc_rule));
	p.count_bytes = sg_up16((size_t)chunk * 2 * sizeof(uint64_t)) + sg_up16((SGC_NCOUNT + 1) * sizeof(uint32_t));
	p.total_bytes = p.state_bytes + 4 * p.plane_bytes + 2 * p.list_bytes + p.hist_bytes + p.rule_bytes + p.count_bytes;
	return p.total_bytes;
}

/* frame_stride in elements, 0 = tight; budget <= 0 = SGC_BUDGET; force_chunk > 0 = that many
 * frames per chunk whatever the budget (still held to the 32-bit pixel id and the grid);
 * force_list > 0 = that list capacity (SG_COSME_LIST: tests of the overflow's plane walk) */
static inline int sg_cosme_plan(const sg_cosme_desc *d, int nframes, int64_t frame_stride, int64_t budget,
		int force_chunk, int force_list, SgCosmePlan &p) {
	p = SgCosmePlan();
	if (!d)
		return sgc_fail(p, SG_ERR_GENERIC, "cosme: no descriptor");
	if (d->width <= 0 || d->height <= 0)
		return sgc_fail(p, SG_ERR_SIZE, "cosme: width or height not positive");
	if ((int64_t)d->width * d->height >= ((int64_t)1 << 31))
		return sgc_fail(p, SG_ERR_SIZE, "cosme: a plane of 2^31 pixels or more");
	if (d->nb_layers < 1 || d->nb_layers > SGC_MAX_LAYERS)
		return sgc_fail(p, SG_ERR_SIZE, "cosme: nb_layers outside [1, 3]");
	if (nframes < 1)
		return sgc_fail(p, SG_ERR_SIZE, "cosme: no frames");
	const int64_t npix = (int64_t)d->width * d->height;
	if (frame_stride == 0)
		frame_stride = npix * d->nb_layers;
	if (frame_stride < npix * d->nb_layers)
		return sgc_fail(p, SG_ERR_SIZE, "cosme: frame_stride below one frame");
	const int step = d->is_cfa ? 2 : 1;
	if (d->width <= step && d->height <= step)
		return sgc_fail(p, SG_ERR_SIZE, "cosme: no pixel of the plane has a neighbour (the reference divides 0 by 0)");
	for (int i = 0; i < 2; i++)
		if (d->sig[i] != d->sig[i] || (d->sig[i] < 0.0 && d->sig[i] != -1.0))
			return sgc_fail(p, SG_ERR_GENERIC, "cosme: a sigma that is NaN, or negative and not -1");
	if (!(d->amount >= 0.0 && d->amount <= 1.0))
		return sgc_fail(p, SG_ERR_GENERIC, "cosme: amount outside [0, 1]");
	p.W = d->width;
	p.H = d->height;
	p.C = d->nb_layers;
	p.nframes = nframes;
	p.is_cfa = d->is_cfa ? 1 : 0;
	p.step = step;
	p.halo = 2 * step;
	p.sig0 = d->sig[0];
	p.sig1 = d->sig[1];
	p.amount = d->amount;
	p.npix = npix;
	p.frame_stride = frame_stride;
	p.tiles_x = (p.W + SGC_TILE_W - 1) / SGC_TILE_W;
	p.tiles_y = (p.H + SGC_TILE_H - 1) / SGC_TILE_H;
	p.in_w = SGC_TILE_W + 2 * p.halo;
	p.in_h = SGC_TILE_H + 2 * p.halo;
	p.lds_tile = (size_t)p.in_w * p.in_h * sizeof(uint16_t);
	p.hist_blocks = (int)((npix + SGC_HIST_CHUNK - 1) / SGC_HIST_CHUNK);
	if (sgc_chunk_bytes(p, 1, force_list) == 0)
		return sgc_fail(p, SG_ERR_SIZE, "cosme: one frame's pixels do not fit a 32-bit id");
	int64_t c = (budget > 0 ? budget : SGC_BUDGET) / (int64_t)p.total_bytes;
	if (force_chunk > 0)
		c = force_chunk;
	if (c > nframes)
		c = nframes;
	if (c > SGC_MAX_Z / p.C)
		c = SGC_MAX_Z / p.C;
	if (c < 1)
		c = 1;
	while (c > 1 && sgc_chunk_bytes(p, c, force_list) == 0)
		c = (c + 1) / 2;
	sgc_chunk_bytes(p, c, force_list);
	p.chunk = (int)c;
	p.nchunks = (nframes + p.chunk - 1) / p.chunk;
	return SG_OK;
}
