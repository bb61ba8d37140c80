/*
 * sg_starmatch_plan.hpp - the host-only plan of a star matching call (include/sirilgpu.h,
 * sg_starmatch), with no HIP in it, so tests/test_starmatch_cpu.py builds and checks it without a GPU:
 *   - the argument checks (each before any device work);
 *   - the frame loop's statuses that need no matching (reference, excluded, too few stars) and the
 *     table of the frames to match, one workgroup each;
 *   - the packing of (xpos, ypos, mag): the reference's first fitted_stars stars, then the first
 *     nbpoints stars of every frame to match, as triples of doubles;
 *   - the LDS bytes of a workgroup (the layout is SgmWork's, stated in sg_starmatch.h) and the grid;
 *   - FWHM_average and the warp plan, which are host work.
 */
#pragma once
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <vector>
#include "sg_host_batch.hpp"
#include "sg_starmatch.h"

#define SGM_LDS_MAX (160 * 1024)	/* a gfx950 workgroup's LDS */

/* one frame to match */
struct SgStarmatchItem {
	int32_t frame;		/* its index in the sequence */
	int32_t n;		/* nbpoints */
	int64_t a_off;		/* its list in the packed doubles */
};

struct SgStarmatchPlan {
	int nframes = 0, ref_image = 0, fitted = 0, nmax = 0;
	size_t lds_bytes = 0;
	unsigned grid = 0, threads = SGM_LANES;
	std::vector<int32_t> status;		/* per frame: what is known without matching, else SG_MATCH_OK */
	std::vector<SgStarmatchItem> items;
	std::vector<double> packed;		/* the reference's triples at 0 */
	size_t packed_bytes = 0, table_bytes = 0, result_bytes = 0, pairs_bytes = 0;
	char err[256] = "";
};

static inline int sgm_fail(SgStarmatchPlan &p, int code, const char *msg) {
	snprintf(p.err, sizeof p.err, "%s", msg);
	return code;
}

static inline void sgm_pack(const sg_star *s, int n, std::vector<double> &out) {
	for (int i = 0; i < n; i++) {
		out.push_back(s[i].xpos);
		out.push_back(s[i].ypos);
		out.push_back(s[i].mag);
	}
}

static inline bool sgm_all_finite(const sg_star *s, int n) {
	for (int i = 0; i < n; i++)
		if (!isfinite(s[i].xpos) || !isfinite(s[i].ypos) || !isfinite(s[i].mag))
			return false;
	return true;
}

/* SG_OK; SG_ERR_SIZE / SG_ERR_GENERIC with p.err for a refusal; a reference with fewer than
 * AT_MATCH_MINPAIRS stars is SG_ERR_GENERIC too (the whole registration fails) */
static inline int sg_starmatch_plan(int nframes, int max_stars, const int32_t *nstars, const sg_star *stars, int ref_image,
		const uint8_t *included, const void *results, int want_pairs, SgStarmatchPlan &p) {
	p = SgStarmatchPlan();
	if (nframes < 1)
		return sgm_fail(p, SG_ERR_SIZE, "starmatch: no frames");
	if (max_stars < 1 || max_stars > SG_STARFIT_MAX_STARS)
		return sgm_fail(p, SG_ERR_SIZE, "starmatch: max_stars outside 1 .. 50000");
	if (!nstars || !stars || !results)
		return sgm_fail(p, SG_ERR_GENERIC, "starmatch: missing star counts, stars or results");
	if (ref_image < 0 || ref_image >= nframes)
		return sgm_fail(p, SG_ERR_GENERIC, "starmatch: ref_image outside the sequence");
	if (included && !included[ref_image])
		return sgm_fail(p, SG_ERR_GENERIC, "starmatch: the reference frame is excluded");
	for (int f = 0; f < nframes; f++)
		if (nstars[f] < 0 || nstars[f] > max_stars)
			return sgm_fail(p, SG_ERR_GENERIC, "starmatch: a star count outside 0 .. max_stars");
	const int nref = nstars[ref_image];
	const int fitted = nref > MAX_STARS_FITTED ? MAX_STARS_FITTED : nref;
	const sg_star *ref = stars + (size_t)ref_image * max_stars;
	if (!sgm_all_finite(ref, fitted))
		return sgm_fail(p, SG_ERR_GENERIC, "starmatch: a reference star's xpos, ypos or mag is not finite");
	for (int f = 0; f < nframes; f++) {
		const int n = nstars[f] < fitted ? nstars[f] : fitted;
		if (f != ref_image && (!included || included[f]) && nstars[f] >= AT_MATCH_MINPAIRS &&
				!sgm_all_finite(stars + (size_t)f * max_stars, n))
			return sgm_fail(p, SG_ERR_GENERIC, "starmatch: a star's xpos, ypos or mag is not finite");
	}
	if (nref < AT_MATCH_MINPAIRS)
		return sgm_fail(p, SG_ERR_GENERIC, "starmatch: there are not enough stars in the reference image to perform alignment");
	p.nframes = nframes;
	p.ref_image = ref_image;
	p.fitted = fitted;
	p.status.assign((size_t)nframes, SG_MATCH_OK);
	sgm_pack(ref, fitted, p.packed);
	for (int f = 0; f < nframes; f++) {
		if (included && !included[f]) {
			p.status[(size_t)f] = SG_MATCH_EXCLUDED;
		} else if (f == ref_image) {
			p.status[(size_t)f] = SG_MATCH_REFERENCE;
		} else if (nstars[f] < AT_MATCH_MINPAIRS) {
			p.status[(size_t)f] = SG_MATCH_FEW_STARS;
		} else {
			SgStarmatchItem it;
			it.frame = f;
			it.n = nstars[f] < fitted ? nstars[f] : fitted;
			it.a_off = (int64_t)p.packed.size();
			sgm_pack(stars + (size_t)f * max_stars, it.n, p.packed);
			p.items.push_back(it);
			if (it.n > p.nmax)
				p.nmax = it.n;
		}
	}
	p.grid = (unsigned)p.items.size();
	p.lds_bytes = p.nmax ? sg_up16(sgm_work_bytes(p.nmax)) : 0;
	if (p.lds_bytes > SGM_LDS_MAX)
		return sgm_fail(p, SG_ERR_GENERIC, "starmatch: the workspace exceeds a workgroup's LDS");
	p.packed_bytes = sg_up16(p.packed.size() * sizeof(double));
	p.table_bytes = sg_up16(p.items.size() * sizeof(SgStarmatchItem));
	p.result_bytes = sg_up16(p.items.size() * sizeof(sg_starmatch_result));
	p.pairs_bytes = want_pairs ? sg_up16(p.items.size() * (size_t)2 * MAX_STARS_FITTED * sizeof(int32_t)) : 0;
	return SG_OK;
}

/* FWHM_average (src/algos/star_finder.c:353-367): float sums in order */
static inline void sgm_fwhm_average(const sg_star *s, int n, float *fx, float *fy) {
	float x = 0.0f, y = 0.0f;
	int i = 0;
	while (i < n) {
		x += (float)s[i].fwhmx;
		y += (float)s[i].fwhmy;
		i++;
	}
	*fx = x / (float)i;
	*fy = y / (float)i;
}

/* the results of the frames that are not matched, and FWHM_average of the reference */
static inline void sgm_fill_unmatched(const SgStarmatchPlan &p, int max_stars, const sg_star *stars, sg_starmatch_result *results) {
	for (int f = 0; f < p.nframes; f++) {
		const int st = p.status[(size_t)f];
		if (st == SG_MATCH_OK)
			continue;
		sgm_result_clear(&results[f], st);
		if (st == SG_MATCH_REFERENCE) {
			results[f].nbpoints = p.fitted;
			results[f].hom[0] = results[f].hom[4] = results[f].hom[8] = 1.0;
			sgm_fwhm_average(stars + (size_t)f * max_stars, p.fitted, &results[f].fwhmx, &results[f].fwhmy);
		}
	}
}

/* the loop's failed / skipped bookkeeping (src/registration/registration.c:653-755) */
static inline int sgm_warp_plan(const sg_starmatch_result *results, int nframes, double *hom, int *action, int *out_slot,
		int *new_total) {
	if (!results || !hom || !action || !out_slot || nframes < 1)
		return -1;
	int failed = 0, skipped = 0;
	for (int f = 0; f < nframes; f++) {
		const int st = results[f].status;
		action[f] = SG_WARP_SKIP;
		out_slot[f] = 0;
		for (int k = 0; k < 9; k++)
			hom[(size_t)f * 9 + k] = 0.0;
		if (st == SG_MATCH_EXCLUDED) {
			skipped++;
		} else if (st == SG_MATCH_OK || st == SG_MATCH_REFERENCE) {
			action[f] = st == SG_MATCH_REFERENCE ? SG_WARP_COPY : SG_WARP_APPLY;
			for (int k = 0; k < 9; k++)
				hom[(size_t)f * 9 + k] = results[f].hom[k];
			out_slot[f] = f - failed - skipped;
		} else {
			failed++;
		}
	}
	if (new_total)
		*new_total = nframes - failed - skipped;
	return 0;
}
