/*
 * sg_starfit_plan.hpp - the host-only plan of a fitted star call (include/sirilgpu.h,
 * sg_findstar_fit*), with no HIP in it, so tests/test_starfit_plan_cpu.py builds and checks it
 * without a GPU: the argument checks (each before any device work, after those of
 * sg_findstar_plan), the box and LDS sizes of k_starfit_fit, its grid, and the bytes of the
 * device-side records.
 */
#pragma once
#include "sg_findstar_plan.hpp"

#define SGS_WAVES 4		/* candidates (waves) per workgroup of k_starfit_fit */

struct SgStarfitPlan {
	SgFindstarPlan find;
	double roundness = 0., norm = 0., scale_x = 1., scale_y = 1.;
	int max_stars = 0, want_candidates = 0;
	int n2 = 0, box_elems = 0;	/* 2r, 4r^2 */
	size_t lds_bytes = 0;		/* SGS_WAVES boxes of uint16 */
	size_t cand_bytes = 0, star_bytes = 0;	/* one record of each kind */
	char err[256] = "";
};

static inline int sgs_fail(SgStarfitPlan &p, int code, const char *msg) {
	snprintf(p.err, sizeof p.err, "%s", msg);
	return code;
}

static inline int sg_starfit_plan(const sg_starfit_desc *d, SgStarfitPlan &p) {
	p = SgStarfitPlan();
	if (!d)
		return sgs_fail(p, SG_ERR_GENERIC, "no descriptor");
	const int rc = sg_findstar_plan(&d->find, p.find);
	if (rc != SG_OK)
		return sgs_fail(p, rc, p.find.err);
	if (d->find.radius > SG_STARFIT_MAX_RADIUS)
		return sgs_fail(p, SG_ERR_GENERIC, "starfit: radius above 32 (the box would not fit the wave's LDS share)");
	if (!isfinite(d->roundness) || !isfinite(d->fwhm_scale_x) || !isfinite(d->fwhm_scale_y))
		return sgs_fail(p, SG_ERR_GENERIC, "starfit: roundness or an FWHM scale not finite");
	if (d->norm != 255. && d->norm != 65535.)
		return sgs_fail(p, SG_ERR_GENERIC, "starfit: norm is neither 255 nor 65535");
	if (d->max_stars < 0 || d->max_stars > SG_STARFIT_MAX_STARS)
		return sgs_fail(p, SG_ERR_GENERIC, "starfit: max_stars outside [0, 50000]");
	p.roundness = d->roundness;
	p.norm = d->norm;
	p.scale_x = d->fwhm_scale_x;
	p.scale_y = d->fwhm_scale_y;
	p.max_stars = d->max_stars;
	p.want_candidates = d->want_candidates != 0;
	p.n2 = 2 * p.find.r;
	p.box_elems = p.n2 * p.n2;
	p.lds_bytes = (size_t)SGS_WAVES * p.box_elems * sizeof(uint16_t);
	p.cand_bytes = sizeof(sg_starfit_cand);
	p.star_bytes = sizeof(sg_star);
	return SG_OK;
}

/* workgroups along x of k_starfit_fit for the chunk's largest stored count (y: the frame) */
static inline unsigned sgs_grid_x(uint64_t most) {
	return (unsigned)((most + SGS_WAVES - 1) / SGS_WAVES);
}
