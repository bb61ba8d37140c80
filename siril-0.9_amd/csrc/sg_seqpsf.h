/*
 * sg_seqpsf.h - the per-frame part of seqpsf (src/io/sequence.c:1627-1820, 1123-1130;
 * src/algos/PSF.c:46-91, 434-559, 583-662; src/core/siril.c:1173-1192;
 * src/algos/statistics.c:47-63, 207-256; src/gui/histogram.c:129-150; src/core/utils.c:60-66) and
 * the second step of register_shift_fwhm (src/registration/registration.c:406-490), host + device,
 * no HIP types: the area rules, the non-zero median of a box, getMedian3x3 on an h x w box, the
 * frame's two fits with the finish of psf_minimiz_angle and psf_global_minimisation, and
 * sg_seqpsf_fit_box, which runs a whole box sequentially.  The start-value walks, both models, the
 * solver (sgp_lm<6> and sgp_lm<7>) and the sequential evaluator are sg_psf.h's.  The kernels of
 * sg_seqpsf.hip call the same functions with a workgroup-wide evaluator, so everything but their
 * sums is checked on the host (tests/test_seqpsf_cpu.py).
 *
 * The box is psf_get_minimisation's gsl_matrix z as uint16, z[i][j] = box[i * w + j]: i < h the
 * matrix rows (image y, bottom-up), j < w the columns (image x).  Not transposed, unlike peaker's.
 *
 * Departure: the literal `while (fabs(angle) > 90) angle -+= 90` gets a bound of SQ_MAX_FOLD steps;
 * a fit needing more reports SG_FIT_NONFINITE.  alpha starts at 0 and makes at most 10 steps, so
 * |angle| > 90 * 9 means a fit that ran away.
 */
#pragma once
#include "sg_psf.h"

#define SQ_MAX_FOLD 8
#define SQ_EPSILON 0.01			/* EPSILON of PSF.c: |SX - SY| below it, no angle fit */
#define SQ_PI 3.14159265358979323846	/* M_PI */

/* ---------------------------------------------------------------- areas (steps 1 and 6) */

/* round_to_int (utils.c:60-66) */
SGP_HD int sq_round_to_int(double x) {
	if (x >= 0.0)
		return (int)(x + 0.5);
	return (int)(x - 0.5);
}

/* enforce_area_in_image (sequence.c:1123-1130) on a copy; w <= W and h <= H */
SGP_HD void sq_enforce_area(int W, int H, int w, int h, int *x, int *y) {
	if (*x < 0)
		*x = 0;
	if (*y < 0)
		*y = 0;
	if (*x + w > W)
		*x = W - w;
	if (*y + h > H)
		*y = H - h;
}

/* the area of a frame of the parallel framings: REGISTERED moves it by the frame's shifts first.
 * The sums are taken in 64 bits and held to the int range the clamp then brings inside anyway. */
SGP_HD void sq_frame_area(int registered, int ax, int ay, int shiftx, int shifty, int W, int H, int w, int h, int *x,
		int *y) {
	int64_t tx = ax, ty = ay;
	if (registered) {
		tx -= shiftx;
		ty += shifty;
	}
	const int64_t lim = (int64_t)1 << 30;
	tx = tx < -lim ? -lim : (tx > lim ? lim : tx);
	ty = ty < -lim ? -lim : (ty > lim ? lim : ty);
	*x = (int)tx;
	*y = (int)ty;
	sq_enforce_area(W, H, w, h, x, y);
}

/* FOLLOW_STAR: the carried (unclamped) area after a frame with a PSF; w / 2 is integer division.
 * xpos / ypos lie inside the image's box plus the fit's wander; values beyond the int range are held. */
SGP_HD void sq_follow_area(double xpos, double ypos, int w, int h, int *x, int *y) {
	const double lim = 1073741824.0;
	const double cx = xpos < -lim ? -lim : (xpos > lim ? lim : xpos), cy = ypos < -lim ? -lim : (ypos > lim ? lim : ypos);
	*x = sq_round_to_int(cx) - w / 2;
	*y = sq_round_to_int(cy) - h / 2;
}

/* ---------------------------------------------------------------- background (step 3) */

/* statistics(STATS_BASIC, STATS_ZERO_NULLCHECK) -> median of the box, sequentially: ngood counts the
 * non-zero pixels; 65536 bins over [0, 65535) leave the value 65535 unbinned; from bin 1, the first
 * bin whose running count exceeds ngood * 0.5, else 0 (also when ngood = 0: background() gives 0.0).
 * Counting selection without the histogram: the value v is the answer when the count of non-zero
 * values <= v first exceeds ngood / 2. */
static inline double sq_bg_box(const uint16_t *box, int n, int64_t *ngood_out) {
	int64_t ngood = 0;
	for (int p = 0; p < n; p++)
		ngood += box[p] != 0;
	*ngood_out = ngood;
	/* bisection on the value: count(0 < z <= v) is monotone in v */
	int lo = 1, hi = 65535;		/* hi = 65535 stands for "no bin" */
	while (lo < hi) {
		const int mid = (lo + hi) / 2;
		int64_t c = 0;
		for (int p = 0; p < n; p++)
			c += box[p] != 0 && box[p] <= mid;
		if (2 * c > ngood)
			hi = mid;
		else
			lo = mid + 1;
	}
	return lo >= 65535 ? 0.0 : (double)lo;
}

/* ---------------------------------------------------------------- start values (step 4) */

/* getMedian3x3 at (row i, column j) of an h x w box; see sgp_median3x3, which this one agrees with
 * wherever that one is defined */
SGP_HD uint16_t sq_median3x3(const uint16_t *box, int h, int w, int i, int j) {
	uint32_t v[8];
	int n = 0;
SGP_UNROLL
	for (int t = 0; t < 9; t++) {
		if (t == 4)
			continue;
		const int y = i + t / 3 - 1, x = j + t % 3 - 1;
		const int in = y >= 0 && y < h && x >= 0 && x < w;
		v[t < 4 ? t : t - 1] = in ? (uint32_t)box[y * w + x] : 0xFFFFFFFFu;	/* outside: sorts last */
		n += in;
	}
	/* n = 8, 5 or 3 in a box of two or more rows and columns; a one-pixel-wide box has n = 2 (the
	 * mean of the padding's last zero and the smaller value) or n = 1 at its ends (that zero) */
	/* the literal reads sorted[8 - n - 1 + (n - 1) / 2] and [8 - n - 1 + n / 2] of the 8 - n zeros
	 * followed by the n values: position q of that array is a zero when q < 8 - n, else the value of
	 * rank q - (8 - n) (ties by position) */
	if (n == 0)
		return 0;	/* a 1 x 1 box, never fitted (n <= 6) */
	const int lhs = 8 - n - 1 + (n - 1) / 2, rhs = 8 - n - 1 + n / 2;
	const int k0 = lhs - (8 - n), k1 = rhs - (8 - n);	/* -1: the padding's last zero */
	uint32_t e0 = 0, e1 = 0;
SGP_UNROLL
	for (int a = 0; a < 8; a++) {
		int rank = 0;
SGP_UNROLL
		for (int b = 0; b < 8; b++)
			rank += (v[b] < v[a]) || (v[b] == v[a] && b < a);
		if (rank == k0)
			e0 = v[a];
		if (rank == k1)
			e1 = v[a];
	}
	return (uint16_t)(lhs == rhs ? e0 : (e0 + e1) / 2u);
}

/* ---------------------------------------------------------------- a frame's fit (steps 4 to 6) */

SGP_HD void sq_frame_clear(sg_seqpsf_frame &o, int status) {
	o.status = status;
	o.angle_fitted = o.iters = o.iters_angle = 0;
	o.area_x = o.area_y = 0;
	o.ngood = 0;
	o.bg = 0.;
SGP_UNROLL
	for (int k = 0; k < 6; k++)
		o.init[k] = o.noangle[k] = 0.;
	o.B = o.A = o.x0 = o.y0 = o.sx = o.sy = o.fwhmx = o.fwhmy = o.angle = o.mag = o.rmse = o.xpos = o.ypos = 0.;
}

template <int NP>
SGP_HD int sq_all_finite(const double x[NP], double ff) {
	double t = ff;
SGP_UNROLL
	for (int k = 0; k < NP; k++)
		t += x[k];
	return sgp_finite(t);
}

/*
 * psf_global_minimisation(z, bg, layer, fit_angle, FALSE), psf_update_units and the hook's xpos /
 * ypos for the box read from the clamped area (area_x, area_y, w, h).  o arrives with area_x / y,
 * ngood, bg and init filled and everything else cleared; o.status receives 0 (a PSF) or SG_FIT_*.
 * ev is an evaluator of sg_psf.h, used at p = 6 and p = 7.
 */
template <class Ev>
SGP_HD void sq_fit(Ev &ev, int w, int h, int fit_angle, double norm, double scale_x, double scale_y, sg_seqpsf_frame &o) {
	const int n = w * h;
	o.status = SG_FIT_NOT_ENOUGH_PIXELS;
	if (n <= 6)
		return;
	double x[7], ff;
SGP_UNROLL
	for (int k = 0; k < 6; k++)
		x[k] = o.init[k];
	x[6] = 0.;
	int it = 0;
	int bad = sgp_lm<6>(ev, x, &ff, &it);
	o.iters = it;
	if (bad || !sq_all_finite<6>(x, ff)) {
		o.status = SG_FIT_NONFINITE;
		return;
	}
SGP_UNROLL
	for (int k = 0; k < 6; k++)
		o.noangle[k] = x[k];
	double angle = 0.;
	if (fit_angle && fabs(x[4] - x[5]) >= SQ_EPSILON) {
		o.angle_fitted = 1;
		bad = sgp_lm<7>(ev, x, &ff, &it);
		o.iters_angle = it;
		if (bad || !sq_all_finite<7>(x, ff)) {
			o.status = SG_FIT_NONFINITE;
			return;
		}
		angle = -x[6] * 180.0 / SQ_PI;
		for (int k = 0; k < SQ_MAX_FOLD && fabs(angle) > 90.0; k++) {
			if (angle > 0.0)
				angle -= 90.0;
			else
				angle += 90.0;
		}
		if (fabs(angle) > 90.0) {
			o.status = SG_FIT_NONFINITE;
			return;
		}
	}
	o.B = x[0];
	o.A = x[1];
	o.x0 = x[2];
	o.y0 = x[3];
	o.sx = x[4];
	o.sy = x[5];
	o.fwhmx = sqrt(x[4] / 2.) * SGP_FWHM_K;
	o.fwhmy = sqrt(x[5] / 2.) * SGP_FWHM_K;
	o.mag = -2.5 * log10(ev.flux(x[0]));
	o.rmse = sqrt(ff / (double)n);
	if (o.sy > o.sx) {
		double t = o.sx;
		o.sx = o.sy;
		o.sy = t;
		t = o.fwhmx;
		o.fwhmx = o.fwhmy;
		o.fwhmy = t;
		if (o.angle_fitted && angle != 0.0) {
			if (angle > 0.0)
				angle -= 90.0;
			else
				angle += 90.0;
		}
	}
	o.angle = angle;
	o.B = o.B / norm;
	o.A = o.A / norm;
	o.rmse = o.rmse / norm;
	o.xpos = o.x0 + (double)o.area_x;
	o.ypos = (double)o.area_y + (double)h - o.y0;
	if (!sgp_finite(o.fwhmx) || !sgp_finite(o.fwhmy) || o.fwhmx <= 0.0 || o.fwhmy <= 0.0) {
		o.status = SG_FIT_BAD_FWHM;
		return;
	}
	o.fwhmx *= scale_x;
	o.fwhmy *= scale_y;
	o.status = SG_FIT_STAR;
}

/* a whole frame's box sequentially: steps 3 to 6 for the box box[i * w + j] read from the clamped
 * area (area_x, area_y, w, h) */
static inline void sg_seqpsf_fit_box(const uint16_t *box, int w, int h, int area_x, int area_y, int fit_angle, double norm,
		double scale_x, double scale_y, sg_seqpsf_frame &o) {
	sq_frame_clear(o, SG_FIT_NOT_ENOUGH_PIXELS);
	o.area_x = area_x;
	o.area_y = area_y;
	int64_t ngood;
	o.bg = sq_bg_box(box, w * h, &ngood);
	o.ngood = ngood;
	sgp_init_box(box, h, w, o.bg, [h, w](const uint16_t *b, int i, int j) { return sq_median3x3(b, h, w, i, j); }, o.init);
	SgPsfSeqEval ev = {box, h, w};
	sq_fit(ev, w, h, fit_angle, norm, scale_x, scale_y, o);
}

/* ---------------------------------------------------------------- shifts (step 8) */

/* register_shift_fwhm's second step from the records; see sg_seqpsf_shifts in include/sirilgpu.h */
static inline int sq_shifts(int nframes, int ref_image, const sg_seqpsf_frame *rec, int *shiftx, int *shifty, double *fwhm,
		int *best_index, double *best_fwhm) {
	for (int f = 0; f < nframes; f++)
		if (rec[f].status != SG_SEQPSF_EXCLUDED && rec[f].status != SG_FIT_STAR)
			return 1;	/* seqpsf aborted: nothing stored */
	const int ref = ref_image < 0 ? 0 : ref_image;
	if (ref >= nframes || rec[ref].status == SG_SEQPSF_EXCLUDED)
		return -1;
	double fwhm_min = rec[ref].fwhmx;
	int fwhm_index = ref;
	for (int f = 0; f < nframes; f++) {
		const int inc = rec[f].status != SG_SEQPSF_EXCLUDED;
		if (fwhm)
			fwhm[f] = inc ? rec[f].fwhmx : 0.;
		if (f == ref || !inc) {
			shiftx[f] = 0;
			shifty[f] = 0;
			continue;
		}
		if (rec[f].fwhmx < fwhm_min && rec[f].fwhmx > 0.0) {
			fwhm_min = rec[f].fwhmx;
			fwhm_index = f;
		}
		shiftx[f] = sq_round_to_int(rec[ref].xpos - rec[f].xpos);
		shifty[f] = sq_round_to_int(rec[f].ypos - rec[ref].ypos);
	}
	if (best_index)
		*best_index = fwhm_index;
	if (best_fwhm)
		*best_fwhm = fwhm_min;
	return 0;
}
