/*
 * sg_seqpsf.h - the per-frame part of seqpsf (src/io/sequence.c:1627-1820, 1123-1130;
 * src/algos/PSF.c:46-157, 229-309, 434-559, 583-662; src/core/siril.c:1173-1192;
 * src/algos/statistics.c:47-63, 207-256; src/gui/histogram.c:129-150; src/core/utils.c:60-66) and
 * the second step of register_shift_fwhm (src/registration/registration.c:406-490), host + device,
 * no HIP types: the area rules, the non-zero median of a box, the start values of psf_init_data on
 * an h x w box, the models and Jacobians of psf_Gaussian_f / _df and psf_Gaussian_f_an / _df_an as
 * sums, lmsder for p = 6 and p = 7 on an evaluator, the finish of psf_minimiz_angle and
 * psf_global_minimisation, and sg_seqpsf_fit_box, which runs a whole box sequentially.  The kernels
 * of sg_seqpsf.hip call the same functions with a workgroup-wide evaluator, so everything but their
 * sums is checked on the host (tests/test_seqpsf_cpu.py).
 *
 * The box is psf_get_minimisation's gsl_matrix z as uint16, z[i][j] = box[i * w + j]: i < h the
 * matrix rows (image y, bottom-up), j < w the columns (image x).  Not transposed, unlike peaker's.
 *
 * The solver is sg_psf.h's (MINPACK lmder / lmpar on the scaled normal equations, Cholesky, every
 * loop with a constant bound), written once for both parameter counts.  sg_psf.h itself is left as
 * it is: k_starfit_fit's code must not move.
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

/* getMedian3x3 at (row i, column j) of an h x w box; see sgp_median3x3 */
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

/* sgp_init_walks on an h x w box: the maximum at (row mi, column mj), filtered value mx */
SGP_HD void sq_init_walks(const uint16_t *box, int h, int w, double bg, int mi, int mj, uint16_t mx, double init[6]) {
	const double zc = (double)box[mi * w + mj] - bg;
	int ii1 = mi, ii2 = mi, jj1 = mj, jj2 = mj;
	while (2.0 * ((double)box[ii1 * w + mj] - bg) > zc && ii1 < h - 1)
		ii1++;
	while (2.0 * ((double)box[ii2 * w + mj] - bg) > zc && ii2 > 0)
		ii2--;
	while (2.0 * ((double)box[mi * w + jj1] - bg) > zc && jj1 < w - 1)
		jj1++;
	while (2.0 * ((double)box[mi * w + jj2] - bg) > zc && jj2 > 0)
		jj2--;
	const double di = (double)((ii1 - ii2) * (ii1 - ii2)), dj = (double)((jj1 - jj2) * (jj1 - jj2));
	init[0] = bg;
	init[1] = (double)mx;
	init[2] = (double)(jj1 + jj2 + 2) / 2.0;
	init[3] = (double)(ii1 + ii2 + 2) / 2.0;
	init[4] = (double)(uint64_t)(dj / 4.0 / SGP_LN2);
	init[5] = (double)(uint64_t)(di / 4.0 / SGP_LN2);
}

/* psf_init_data sequentially: the first maximum of the filtered box in row-major order */
static inline void sq_init_box(const uint16_t *box, int h, int w, double bg, double init[6]) {
	int best = 0;
	uint16_t mx = 0;
	for (int p = 0; p < h * w; p++) {
		const uint16_t m = sq_median3x3(box, h, w, p / w, p % w);
		if (p == 0 || m > mx) {
			mx = m;
			best = p;
		}
	}
	sq_init_walks(box, h, w, bg, best / w, best % w, mx, init);
}

/* ---------------------------------------------------------------- the models as sums */

/* J^T J (upper triangle, row-major), J^T f and |f|^2 for NP parameters: 21 + 6 + 1 or 28 + 7 + 1 */
template <int NP>
struct SqSums {
	double a[NP * (NP + 1) / 2], g[NP], ff;
};

template <int NP>
SGP_HD void sq_sums_zero(SqSums<NP> &s) {
SGP_UNROLL
	for (int k = 0; k < NP * (NP + 1) / 2; k++)
		s.a[k] = 0.;
SGP_UNROLL
	for (int k = 0; k < NP; k++)
		s.g[k] = 0.;
	s.ff = 0.;
}

template <int NP>
SGP_HD int sq_sums_finite(const SqSums<NP> &s) {
	double t = s.ff;
SGP_UNROLL
	for (int k = 0; k < NP * (NP + 1) / 2; k++)
		t += s.a[k];
SGP_UNROLL
	for (int k = 0; k < NP; k++)
		t += s.g[k];
	return sgp_finite(t);
}

template <int NP>
SGP_HD void sq_accum(const double J[NP], double r, SqSums<NP> &s) {
	int k = 0;
SGP_UNROLL
	for (int i = 0; i < NP; i++) {
SGP_UNROLL
		for (int j = i; j < NP; j++)
			s.a[k++] += J[i] * J[j];
		s.g[i] += J[i] * r;
	}
	s.ff += r * r;
}

/* what a model evaluation at x shares among its pixels: cos and sin of alpha for p = 7 */
template <int NP>
struct SqModel {
	double ca, sa;
};

template <int NP>
SGP_HD SqModel<NP> sq_model(const double x[NP]) {
	SqModel<NP> m;
	if (NP == 7) {
		m.ca = cos(x[NP - 1]);
		m.sa = sin(x[NP - 1]);
	} else {
		m.ca = 1.;
		m.sa = 0.;
	}
	return m;
}

/* the residual at pixel (row i, column j) of value z: tx = j + 1, ty = i + 1.  p = 6:
 * psf_Gaussian_f; p = 7: psf_Gaussian_f_an as written (tmpx = cos a (j + 1 - x0) - sin a (i + 1 - y0)
 * + x0, then tmpx - x0 again) */
template <int NP>
SGP_HD double sq_resid(const double x[NP], const SqModel<NP> &m, double tx, double ty, double z) {
	double dx, dy;
	if (NP == 7) {
		const double tmpx = m.ca * (tx - x[2]) - m.sa * (ty - x[3]) + x[2];
		const double tmpy = m.sa * (tx - x[2]) + m.ca * (ty - x[3]) + x[3];
		dx = tmpx - x[2];
		dy = tmpy - x[3];
	} else {
		dx = tx - x[2];
		dy = ty - x[3];
	}
	const double c = exp(-(dx * dx / x[4] + dy * dy / x[5]));
	return x[0] + x[1] * c - z;
}

/* residual and Jacobian row (sigma = 1) at one pixel, added to the sums; one exp.  p = 7 is
 * psf_Gaussian_df_an literally: columns 2 and 3 keep their cos(alpha) factor (the derivative with
 * respect to x0 / y0 of the rotated coordinates is not that, the reference's formula is the
 * contract), column 6 as written */
template <int NP>
SGP_HD void sq_pixel(const double x[NP], const SqModel<NP> &m, double tx, double ty, double z, SqSums<NP> &s) {
	double J[NP], dx, dy;
	if (NP == 7) {
		const double tmpx = m.ca * (tx - x[2]) - m.sa * (ty - x[3]) + x[2];
		const double tmpy = m.sa * (tx - x[2]) + m.ca * (ty - x[3]) + x[3];
		dx = tmpx - x[2];
		dy = tmpy - x[3];
	} else {
		dx = tx - x[2];
		dy = ty - x[3];
	}
	const double c = exp(-(dx * dx / x[4] + dy * dy / x[5]));
	const double r = x[0] + x[1] * c - z;
	J[0] = 1.;
	J[1] = c;
	J[2] = x[1] * c * 2 * dx / x[4];
	J[3] = x[1] * c * 2 * dy / x[5];
	J[4] = x[1] * c * (dx * dx) / (x[4] * x[4]);
	J[5] = x[1] * c * (dy * dy) / (x[5] * x[5]);
	if (NP == 7) {
		J[2] = J[2] * m.ca;
		J[3] = J[3] * m.ca;
		const double derx = -m.sa * (tx - x[2]) - m.ca * (ty - x[3]);
		const double dery = m.ca * (tx - x[2]) - m.sa * (ty - x[3]);
		J[NP - 1] = -x[1] * c * (2 * dx / x[4] * derx + 2 * dy / x[5] * dery);
	}
	sq_accum<NP>(J, r, s);
}

/* ---------------------------------------------------------------- NP x NP linear algebra (sg_psf.h's) */

template <int NP>
SGP_HD int sq_chol(const double At[NP][NP], double par, double L[NP][NP], double ri[NP]) {
	int ok = 1;
SGP_UNROLL
	for (int j = 0; j < NP; j++) {
		double d = At[j][j] + par;
SGP_UNROLL
		for (int k = 0; k < j; k++)
			d -= L[j][k] * L[j][k];
		if (!(d > 0.))
			ok = 0;
		const double l = sqrt(d), rl = 1. / l;
		L[j][j] = l;
		ri[j] = rl;
SGP_UNROLL
		for (int i = j + 1; i < NP; i++) {
			double v = At[i][j];
SGP_UNROLL
			for (int k = 0; k < j; k++)
				v -= L[i][k] * L[j][k];
			L[i][j] = v * rl;
		}
	}
	return ok;
}

template <int NP>
SGP_HD void sq_fwd(const double L[NP][NP], const double ri[NP], double w[NP]) {
SGP_UNROLL
	for (int i = 0; i < NP; i++) {
		double v = w[i];
SGP_UNROLL
		for (int k = 0; k < i; k++)
			v -= L[i][k] * w[k];
		w[i] = v * ri[i];
	}
}

template <int NP>
SGP_HD void sq_bwd(const double L[NP][NP], const double ri[NP], double w[NP]) {
SGP_UNROLL
	for (int i = NP - 1; i >= 0; i--) {
		double v = w[i];
SGP_UNROLL
		for (int k = i + 1; k < NP; k++)
			v -= L[k][i] * w[k];
		w[i] = v * ri[i];
	}
}

template <int NP>
SGP_HD double sq_norm(const double v[NP]) {
	double t = 0.;
SGP_UNROLL
	for (int k = 0; k < NP; k++)
		t += v[k] * v[k];
	return sqrt(t);
}

template <int NP>
SGP_HD double sq_solve(const double L[NP][NP], const double ri[NP], const double gt[NP], double y[NP], double *phider) {
SGP_UNROLL
	for (int k = 0; k < NP; k++)
		y[k] = gt[k];
	sq_fwd<NP>(L, ri, y);
	sq_bwd<NP>(L, ri, y);
	const double n = sq_norm<NP>(y);
	double w[NP];
SGP_UNROLL
	for (int k = 0; k < NP; k++)
		w[k] = y[k] / n;
	sq_fwd<NP>(L, ri, w);
	const double wn = sq_norm<NP>(w);
	*phider = wn * wn;
	return n;
}

/* MINPACK lmpar in the scaled variables; see sgp_lmpar */
template <int NP>
SGP_HD void sq_lmpar(const double At[NP][NP], const double gt[NP], double delta, double *par_io, double y[NP]) {
	double L[NP][NP], ri[NP];
	double par = *par_io, par_lower = 0., phider, dxnorm, fp;
	if (sq_chol<NP>(At, 0., L, ri)) {
		dxnorm = sq_solve<NP>(L, ri, gt, y, &phider);
		fp = dxnorm - delta;
		if (fp <= 0.1 * delta) {
			*par_io = 0.;
			return;
		}
		par_lower = phider > 0. ? fp / (delta * phider) : 0.;
	} else {
		dxnorm = INFINITY;
		fp = INFINITY;
	}
	const double gnorm = sq_norm<NP>(gt);
	double par_upper = gnorm / delta;
	if (par_upper == 0.)
		par_upper = DBL_MIN / (delta < 0.1 ? delta : 0.1);
	if (par > par_upper)
		par = par_upper;
	else if (par < par_lower)
		par = par_lower;
	if (par == 0.)
		par = gnorm / dxnorm;
	for (int it = 1;; it++) {
		if (par == 0.) {
			par = 0.001 * par_upper;
			if (par < DBL_MIN)
				par = DBL_MIN;
		}
		if (!sq_chol<NP>(At, par, L, ri)) {
SGP_UNROLL
			for (int k = 0; k < NP; k++)
				y[k] = NAN;
			break;
		}
		dxnorm = sq_solve<NP>(L, ri, gt, y, &phider);
		const double fp_old = fp;
		fp = dxnorm - delta;
		if (fabs(fp) <= 0.1 * delta || (par_lower == 0. && fp <= fp_old && fp_old < 0.) || it == SGP_MAX_LMPAR)
			break;
		const double par_c = fp / (delta * phider);
		if (fp > 0.) {
			if (par > par_lower)
				par_lower = par;
		} else if (fp < 0.) {
			if (par < par_upper)
				par_upper = par;
		}
		par = par + par_c > par_lower ? par + par_c : par_lower;
	}
	*par_io = par;
}

SGP_HD int sq_tri(int np, int i, int j) {	/* index of (i, j), i <= j, in SqSums::a */
	return i * np - i * (i - 1) / 2 + (j - i);
}

/* lmsder on an evaluator, p = NP: ev.full(x, sums) gives the sums at x, ev.resid<NP>(x) gives
 * |f(x)|^2; see sgp_lm.  MAX_ITER_NO_ANGLE = MAX_ITER_ANGLE = 10. */
template <int NP, class Ev>
SGP_HD int sq_lm(Ev &ev, double x[NP], double *ff_out, int *iters) {
	SqSums<NP> s;
	double diag[NP], At[NP][NP], gt[NP], y[NP], p[NP], xt[NP];
	*iters = 0;
	*ff_out = NAN;
	ev.template full<NP>(x, s);
	if (!sq_sums_finite<NP>(s))
		return 1;
	double xn = 0.;
SGP_UNROLL
	for (int k = 0; k < NP; k++) {
		diag[k] = sqrt(s.a[sq_tri(NP, k, k)]);
		if (diag[k] == 0.)
			diag[k] = 1.;
		xn += (diag[k] * x[k]) * (diag[k] * x[k]);
	}
	xn = sqrt(xn);
	double delta = xn == 0. ? 100. : 100. * xn, par = 0., ff = s.ff;
	int first = 1;
	for (int outer = 1; outer <= SGP_MAX_ITER; outer++) {
		*iters = outer;
		const double fnorm = sqrt(ff);
		if (fnorm == 0.)
			break;
SGP_UNROLL
		for (int i = 0; i < NP; i++) {
			gt[i] = s.g[i] / diag[i];
SGP_UNROLL
			for (int j = 0; j < NP; j++)
				At[i][j] = s.a[i <= j ? sq_tri(NP, i, j) : sq_tri(NP, j, i)] / (diag[i] * diag[j]);
		}
		int accepted = 0;
		for (int inner = 0; inner < SGP_MAX_INNER && !accepted; inner++) {
			sq_lmpar<NP>(At, gt, delta, &par, y);
			const double pnorm = sq_norm<NP>(y);
			if (!sgp_finite(pnorm))
				break;
SGP_UNROLL
			for (int k = 0; k < NP; k++) {
				p[k] = -(y[k] / diag[k]);
				xt[k] = x[k] + p[k];
			}
			if (first && pnorm < delta)
				delta = pnorm;
			const double ff1 = ev.template resid<NP>(xt), fnorm1 = sqrt(ff1);
			double actred = -1.;
			if (0.1 * fnorm1 < fnorm) {
				const double u = fnorm1 / fnorm;
				actred = 1. - u * u;
			}
			double q = 0.;
SGP_UNROLL
			for (int i = 0; i < NP; i++) {
				double r = 0.;
SGP_UNROLL
				for (int j = 0; j < NP; j++)
					r += At[i][j] * y[j];
				q += y[i] * r;
			}
			const double t1 = sqrt(q > 0. ? q : 0.) / fnorm, t2 = sqrt(par) * pnorm / fnorm;
			const double prered = t1 * t1 + t2 * t2 / 0.5, dirder = -(t1 * t1 + t2 * t2);
			const double ratio = prered > 0. ? actred / prered : 0.;
			if (ratio > 0.25) {
				if (par == 0. || ratio >= 0.75) {
					delta = pnorm / 0.5;
					par *= 0.5;
				}
			} else {
				double temp = actred >= 0. ? 0.5 : 0.5 * dirder / (dirder + 0.5 * actred);
				if (0.1 * fnorm1 >= fnorm || temp < 0.1)
					temp = 0.1;
				delta = temp * (delta < pnorm / 0.1 ? delta : pnorm / 0.1);
				par /= temp;
			}
			if (ratio >= 1e-4) {
SGP_UNROLL
				for (int k = 0; k < NP; k++)
					x[k] = xt[k];
				ev.template full<NP>(x, s);
				ff = s.ff;
				if (!sq_sums_finite<NP>(s))
					return 1;
				first = 0;
SGP_UNROLL
				for (int k = 0; k < NP; k++) {
					const double c = sqrt(s.a[sq_tri(NP, k, k)]);
					if (c > diag[k])
						diag[k] = c;
				}
				accepted = 1;
			}
		}
		if (!accepted)
			break;
		int conv = 1;	/* gsl_multifit_test_delta(dx, x, 1e-4, 1e-4) */
SGP_UNROLL
		for (int k = 0; k < NP; k++)
			if (!(fabs(p[k]) < 1e-4 + 1e-4 * fabs(x[k])))
				conv = 0;
		if (conv)
			break;
	}
	*ff_out = ff;
	return 0;
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
 * ev gives full / resid for p = 6 and p = 7 and flux(B), the sum of z - B.
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
	int bad = sq_lm<6>(ev, x, &ff, &it);
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
		bad = sq_lm<7>(ev, x, &ff, &it);
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

/* the sequential evaluator: every sum in matrix order */
struct SqSeqEval {
	const uint16_t *box;
	int h, w;
	template <int NP>
	SGP_HD_MEMBER void full(const double *x, SqSums<NP> &s) const {
		sq_sums_zero<NP>(s);
		const SqModel<NP> m = sq_model<NP>(x);
		for (int i = 0; i < h; i++)
			for (int j = 0; j < w; j++)
				sq_pixel<NP>(x, m, (double)(j + 1), (double)(i + 1), (double)box[i * w + j], s);
	}
	template <int NP>
	SGP_HD_MEMBER double resid(const double *x) const {
		const SqModel<NP> m = sq_model<NP>(x);
		double ff = 0.;
		for (int i = 0; i < h; i++)
			for (int j = 0; j < w; j++) {
				const double r = sq_resid<NP>(x, m, (double)(j + 1), (double)(i + 1), (double)box[i * w + j]);
				ff += r * r;
			}
		return ff;
	}
	SGP_HD_MEMBER double flux(double B) const {
		double t = 0.;
		for (int p = 0; p < h * w; p++)
			t += (double)box[p] - B;
		return t;
	}
};

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
	sq_init_box(box, h, w, o.bg, o.init);
	SqSeqEval ev = {box, h, w};
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
