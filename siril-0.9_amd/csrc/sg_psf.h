/*
 * sg_psf.h - the PSF fit of peaker (src/algos/star_finder.c:200-247) and of seqpsf, host + device,
 * no HIP types (src/algos/PSF.c:46-157, 160-309, 314-428, 620-662): the start values of
 * psf_init_data on an h x w box, the models and Jacobians of psf_Gaussian_f / _df (p = 6) and
 * psf_Gaussian_f_an / _df_an (p = 7) as sums, the Levenberg-Marquardt iteration of GSL's lmsder
 * (MINPACK lmder / lmpar) restated on the p x p normal equations, and the sequential evaluator.
 * All of it is written once, with the parameter count NP as a template argument; sg_seqpsf.h adds
 * what belongs to seqpsf alone.  Then peaker's own part: the finish of psf_minimiz_no_angle /
 * psf_global_minimisation, psf_update_units as two factors, is_star, and sg_psf_fit_box, which runs
 * a whole box sequentially.  k_starfit_fit (sg_findstar.hip) calls the same functions with a
 * lane-parallel evaluator, so everything but its sums is checked on the host
 * (tests/test_psf_cpu.py).
 *
 * peaker's box is its gsl_matrix z as uint16, z[i][j] = box[i * n2 + j] with n2 = 2r: rows run
 * along image x, and the model's x0 belongs to the column index j (image y).  Kept as it is.
 *
 * The solver works on S = (J^T J, J^T f, |f|^2), never on J itself, and in the scaled variables
 * y = D p, At = D^-1 J^T J D^-1, gt = D^-1 J^T f, where D = diag is lmder's column scaling.  With
 * M = At + par I = L L^T (Cholesky, no pivoting: the scaling brings the diagonal to 1 or below),
 * lmpar's quantities are |D p| = |y|, the Newton correction |R^-T P^T D^2 p / |D p||^2 =
 * |L^-1 y / |y||^2 and |J p|^2 = y^T At y.  A factorisation that meets a pivot that is not
 * positive (rank-deficient J, or a value that is not finite) takes lmpar's rank-deficient branch:
 * no Newton step, lower bound 0.
 * Every loop has a constant bound: 10 outer iterations, 10 trial steps each, 10 lmpar refinements.
 *
 * An evaluator gives ev.full<NP>(x, sums), the sums at x, ev.resid<NP>(x), |f(x)|^2, and
 * ev.flux(B), the sum of z - B.
 */
#pragma once
#include <math.h>
#include <stdint.h>
#include <float.h>
#include "../../include/sirilgpu.h"

#if defined(__HIPCC__)
#define SGP_HD __host__ __device__ static inline
#define SGP_HD_MEMBER __host__ __device__ inline
#else
#define SGP_HD static inline
#define SGP_HD_MEMBER inline
#endif
/* the NP x NP loops are unrolled on the device so that their arrays stay in registers */
#if defined(__HIP_DEVICE_COMPILE__)
#define SGP_UNROLL _Pragma("unroll")
#else
#define SGP_UNROLL
#endif

#define SGP_NP 6			/* B, A, x0, y0, SX, SY; the angle fit adds alpha */
#define SGP_MAX_ITER 10			/* MAX_ITER_NO_ANGLE = MAX_ITER_ANGLE */
#define SGP_MAX_INNER 10		/* lmsder's trial steps per iteration */
#define SGP_MAX_LMPAR 10
#define SGP_LN2 0.6931471805599453	/* log(2.0) */
#define SGP_FWHM_K 2.3548200450309493	/* 2 * sqrt(log(2.) * 2) */

/* ---------------------------------------------------------------- the models as sums */

/* J^T J (upper triangle, row-major: (0,0) (0,1) .. (0,NP-1) (1,1) ..), J^T f and |f|^2:
 * 21 + 6 + 1 or 28 + 7 + 1 doubles */
template <int NP>
struct SgPsfSums {
	double a[NP * (NP + 1) / 2], g[NP], ff;
};

template <int NP>
SGP_HD void sgp_sums_zero(SgPsfSums<NP> &s) {
SGP_UNROLL
	for (int k = 0; k < NP * (NP + 1) / 2; k++)
		s.a[k] = 0.;
SGP_UNROLL
	for (int k = 0; k < NP; k++)
		s.g[k] = 0.;
	s.ff = 0.;
}

SGP_HD int sgp_finite(double v) {
	return v - v == 0.;
}

template <int NP>
SGP_HD int sgp_sums_finite(const SgPsfSums<NP> &s) {
	double t = s.ff;
SGP_UNROLL
	for (int k = 0; k < NP * (NP + 1) / 2; k++)
		t += s.a[k];
SGP_UNROLL
	for (int k = 0; k < NP; k++)
		t += s.g[k];
	return sgp_finite(t);
}

/* a pixel's residual r and Jacobian row J added to the sums */
template <int NP>
SGP_HD void sgp_accum(const double J[NP], double r, SgPsfSums<NP> &s) {
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
struct SgPsfModel {
	double ca, sa;
};

template <int NP>
SGP_HD SgPsfModel<NP> sgp_model(const double x[NP]) {
	SgPsfModel<NP> m;
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
SGP_HD double sgp_resid(const double x[NP], const SgPsfModel<NP> &m, double tx, double ty, double z) {
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

/* residual and Jacobian row (sigma = 1) at one pixel, added to the sums; one exp.  p = 6:
 * psf_Gaussian_df; p = 7 is psf_Gaussian_df_an literally: columns 2 and 3 keep their cos(alpha)
 * factor (the derivative with respect to x0 / y0 of the rotated coordinates is not that, the
 * reference's formula is the contract), column 6 as written */
template <int NP>
SGP_HD void sgp_pixel(const double x[NP], const SgPsfModel<NP> &m, double tx, double ty, double z, SgPsfSums<NP> &s) {
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
	sgp_accum<NP>(J, r, s);
}

/* ---------------------------------------------------------------- start values (psf_init_data) */

/* getMedian3x3 of a 2r x 2r box at (row i, column j): the neighbours inside the box sorted together
 * with zero padding, read from the offset 8 - n - 1: the mean of the 3rd and 4th smallest of 8, the
 * 2nd smallest of 5, the smallest of 3; truncated to WORD.
 * Not shared with sq_median3x3 (n = 1 and 2 too): that one makes k_starfit_fit's code longer. */
SGP_HD uint16_t sgp_median3x3(const uint16_t *box, int n2, int i, int j) {
	uint32_t v[8];
	int n = 0;
SGP_UNROLL
	for (int t = 0; t < 9; t++) {
		if (t == 4)
			continue;
		const int y = i + t / 3 - 1, x = j + t % 3 - 1;
		const int in = y >= 0 && y < n2 && x >= 0 && x < n2;
		v[t < 4 ? t : t - 1] = in ? (uint32_t)box[y * n2 + x] : 0xFFFFFFFFu;	/* outside: sorts last */
		n += in;
	}
	/* the element of rank k (ties by position) */
	const int k0 = n == 8 ? 2 : (n == 5 ? 1 : 0);
	uint32_t e0 = 0, e1 = 0;
SGP_UNROLL
	for (int a = 0; a < 8; a++) {
		int rank = 0;
SGP_UNROLL
		for (int b = 0; b < 8; b++)
			rank += (v[b] < v[a]) || (v[b] == v[a] && b < a);
		if (rank == k0)
			e0 = v[a];
		if (rank == k0 + 1)
			e1 = v[a];
	}
	return (uint16_t)(n == 8 ? (e0 + e1) / 2u : e0);	/* (WORD)((a + b) / 2.) of integers */
}

/* the four half-maximum walks from the maximum (row mi, column mj, filtered value mx) on the
 * UNFILTERED h x w box against bg, and x_init = {bg, max, (jj1 + jj2 + 2) / 2, (ii1 + ii2 + 2) / 2,
 * (size_t)(SQR(jj1 - jj2) / 4 / log 2), (size_t)(SQR(ii1 - ii2) / 4 / log 2)} */
SGP_HD void sgp_init_walks(const uint16_t *box, int h, int w, double bg, int mi, int mj, uint16_t mx, double init[SGP_NP]) {
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

/* psf_init_data, sequentially: the first maximum of the median-filtered box in row-major order;
 * median(box, i, j) is the box's getMedian3x3 */
template <class Median>
static inline void sgp_init_box(const uint16_t *box, int h, int w, double bg, Median median, double init[SGP_NP]) {
	int best = 0;
	uint16_t mx = 0;
	for (int p = 0; p < h * w; p++) {
		const uint16_t m = median(box, p / w, p % w);
		if (p == 0 || m > mx) {
			mx = m;
			best = p;
		}
	}
	sgp_init_walks(box, h, w, bg, best / w, best % w, mx, init);
}

/* ---------------------------------------------------------------- NP x NP linear algebra */

/* L L^T = At + par I, ri[j] = 1 / L[j][j] (the solves multiply by it: NP divisions a
 * factorisation instead of NP (NP - 1) / 2, none in a solve); 0 when a pivot is not positive */
template <int NP>
SGP_HD int sgp_chol(const double At[NP][NP], double par, double L[NP][NP], double ri[NP]) {
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

/* w <- L^-1 w */
template <int NP>
SGP_HD void sgp_fwd(const double L[NP][NP], const double ri[NP], double w[NP]) {
SGP_UNROLL
	for (int i = 0; i < NP; i++) {
		double v = w[i];
SGP_UNROLL
		for (int k = 0; k < i; k++)
			v -= L[i][k] * w[k];
		w[i] = v * ri[i];
	}
}

/* w <- L^-T w */
template <int NP>
SGP_HD void sgp_bwd(const double L[NP][NP], const double ri[NP], double w[NP]) {
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
SGP_HD double sgp_norm(const double v[NP]) {
	double t = 0.;
SGP_UNROLL
	for (int k = 0; k < NP; k++)
		t += v[k] * v[k];
	return sqrt(t);
}

/* y = (At + par I)^-1 gt through L; |L^-1 (y / |y|)|^2 in *phider.  Returns |y|. */
template <int NP>
SGP_HD double sgp_solve(const double L[NP][NP], const double ri[NP], const double gt[NP], double y[NP], double *phider) {
SGP_UNROLL
	for (int k = 0; k < NP; k++)
		y[k] = gt[k];
	sgp_fwd<NP>(L, ri, y);
	sgp_bwd<NP>(L, ri, y);
	const double n = sgp_norm<NP>(y);
	double w[NP];
SGP_UNROLL
	for (int k = 0; k < NP; k++)
		w[k] = y[k] / n;
	sgp_fwd<NP>(L, ri, w);
	const double wn = sgp_norm<NP>(w);
	*phider = wn * wn;
	return n;
}

/* MINPACK lmpar in the scaled variables: the step y = D p (to be taken downhill, p = -D^-1 y) and
 * the Levenberg-Marquardt parameter for the region |y| <= delta */
template <int NP>
SGP_HD void sgp_lmpar(const double At[NP][NP], const double gt[NP], double delta, double *par_io, double y[NP]) {
	double L[NP][NP], ri[NP];
	double par = *par_io, par_lower = 0., phider, dxnorm, fp;
	if (sgp_chol<NP>(At, 0., L, ri)) {
		dxnorm = sgp_solve<NP>(L, ri, gt, y, &phider);	/* the Gauss-Newton step */
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
	const double gnorm = sgp_norm<NP>(gt);
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
		if (!sgp_chol<NP>(At, par, L, ri)) {	/* not finite: the trial step is refused by its caller */
SGP_UNROLL
			for (int k = 0; k < NP; k++)
				y[k] = NAN;
			break;
		}
		dxnorm = sgp_solve<NP>(L, ri, gt, y, &phider);
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

/* ---------------------------------------------------------------- the fit */

SGP_HD int sgp_tri(int np, int i, int j) {	/* index of (i, j), i <= j, in SgPsfSums<np>::a */
	return i * np - i * (i - 1) / 2 + (j - i);
}

/* lmsder on an evaluator, p = NP.  x holds the start values and receives the result; *ff = |f|^2
 * at the final x; *iters = outer iterations made.  Returns 0, or 1 when a value at an accepted
 * point is not finite. */
template <int NP, class Ev>
SGP_HD int sgp_lm(Ev &ev, double x[NP], double *ff_out, int *iters) {
	SgPsfSums<NP> s;
	double diag[NP], At[NP][NP], gt[NP], y[NP], p[NP], xt[NP];
	*iters = 0;
	*ff_out = NAN;
	ev.template full<NP>(x, s);
	if (!sgp_sums_finite<NP>(s))
		return 1;
	double xn = 0.;
SGP_UNROLL
	for (int k = 0; k < NP; k++) {
		diag[k] = sqrt(s.a[sgp_tri(NP, k, k)]);
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
		if (fnorm == 0.)	/* lmsder returns at once; dx = 0 meets the delta test */
			break;
SGP_UNROLL
		for (int i = 0; i < NP; i++) {
			gt[i] = s.g[i] / diag[i];
SGP_UNROLL
			for (int j = 0; j < NP; j++)
				At[i][j] = s.a[i <= j ? sgp_tri(NP, i, j) : sgp_tri(NP, j, i)] / (diag[i] * diag[j]);
		}
		int accepted = 0;
		for (int inner = 0; inner < SGP_MAX_INNER && !accepted; inner++) {
			sgp_lmpar<NP>(At, gt, delta, &par, y);
			const double pnorm = sgp_norm<NP>(y);
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
			double q = 0.;	/* |J p|^2 */
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
				if (!sgp_sums_finite<NP>(s))
					return 1;
				first = 0;
SGP_UNROLL
				for (int k = 0; k < NP; k++) {
					const double c = sqrt(s.a[sgp_tri(NP, k, k)]);
					if (c > diag[k])
						diag[k] = c;
				}
				accepted = 1;
			}
		}
		if (!accepted)	/* "no progress": the fit stops with its current x */
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

/* the sequential evaluator of an h x w box: every sum in matrix order */
struct SgPsfSeqEval {
	const uint16_t *box;
	int h, w;
	template <int NP>
	SGP_HD_MEMBER void full(const double *x, SgPsfSums<NP> &s) const {
		sgp_sums_zero<NP>(s);
		const SgPsfModel<NP> m = sgp_model<NP>(x);
		for (int i = 0; i < h; i++)
			for (int j = 0; j < w; j++)
				sgp_pixel<NP>(x, m, (double)(j + 1), (double)(i + 1), (double)box[i * w + j], s);
	}
	template <int NP>
	SGP_HD_MEMBER double resid(const double *x) const {
		const SgPsfModel<NP> m = sgp_model<NP>(x);
		double ff = 0.;
		for (int i = 0; i < h; i++)
			for (int j = 0; j < w; j++) {
				const double r = sgp_resid<NP>(x, m, (double)(j + 1), (double)(i + 1), (double)box[i * w + j]);
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

/* ---------------------------------------------------------------- peaker: finish and is_star */

/* the fitted fields shared by sg_star and sg_starfit_cand */
struct SgPsfFit {
	double B, A, x0, y0, sx, sy, fwhmx, fwhmy, mag, rmse, xpos, ypos;
	int iters, status, failed_test;
};

/* is_star (star_finder.c:59-78): 0 for a star, else the number of the test that failed */
SGP_HD int sgp_is_star(const SgPsfFit &r, double roundness) {
	if (isnan(r.fwhmx) || isnan(r.fwhmy))
		return 1;
	if (isnan(r.x0) || isnan(r.y0))
		return 2;
	if (isnan(r.mag))
		return 3;
	if ((r.x0 <= 0.0) || (r.y0 <= 0.0))
		return 4;
	if (r.A < 0.01)
		return 5;
	if (r.sx > 200 || r.sy > 200)
		return 6;
	if (r.fwhmx <= 0.0 || r.fwhmy <= 0.0)
		return 7;
	if ((r.fwhmy / r.fwhmx) < roundness)
		return 8;
	return 0;
}

/* psf_minimiz_no_angle's output, the sx / sy swap and normalisation of psf_global_minimisation, its
 * FWHM test, psf_update_units as the two factors, is_star and peaker's xpos / ypos.  intensity is
 * the sum of (z - B), ff = |f|^2 at x, n the pixels; (cx, cy) the candidate. */
SGP_HD void sgp_finish(const double x[SGP_NP], double ff, double intensity, int n, int r, int cx, int cy, double norm,
		double scale_x, double scale_y, double roundness, SgPsfFit &o) {
	o.B = x[0];
	o.A = x[1];
	o.x0 = x[2];
	o.y0 = x[3];
	o.sx = x[4];
	o.sy = x[5];
	o.fwhmx = sqrt(x[4] / 2.) * SGP_FWHM_K;
	o.fwhmy = sqrt(x[5] / 2.) * SGP_FWHM_K;
	o.mag = -2.5 * log10(intensity);
	o.rmse = sqrt(ff / (double)n);
	if (o.sy > o.sx) {
		double t = o.sx;
		o.sx = o.sy;
		o.sy = t;
		t = o.fwhmx;
		o.fwhmx = o.fwhmy;
		o.fwhmy = t;
	}
	o.B = o.B / norm;
	o.A = o.A / norm;
	o.rmse = o.rmse / norm;
	o.xpos = (double)cx + o.x0 - (double)r - 1.;
	o.ypos = (double)cy + o.y0 - (double)r - 1.;
	o.failed_test = 0;
	if (!sgp_finite(o.fwhmx) || !sgp_finite(o.fwhmy) || o.fwhmx <= 0.0 || o.fwhmy <= 0.0) {
		o.status = SG_FIT_BAD_FWHM;
		return;
	}
	o.fwhmx *= scale_x;
	o.fwhmy *= scale_y;
	o.failed_test = sgp_is_star(o, roundness);
	o.status = o.failed_test ? SG_FIT_NOT_STAR : SG_FIT_STAR;
}

SGP_HD void sgp_fit_clear(SgPsfFit &o, int status) {
	o.B = o.A = o.x0 = o.y0 = o.sx = o.sy = o.fwhmx = o.fwhmy = o.mag = o.rmse = o.xpos = o.ypos = 0.;
	o.iters = 0;
	o.status = status;
	o.failed_test = 0;
}

/* peaker's fit after the start values, on any evaluator */
template <class Ev>
SGP_HD void sgp_fit(Ev &ev, const double init[SGP_NP], int n2, int cx, int cy, double norm, double scale_x,
		double scale_y, double roundness, SgPsfFit &o) {
	const int n = n2 * n2;
	sgp_fit_clear(o, SG_FIT_NOT_ENOUGH_PIXELS);
	if (n <= SGP_NP)
		return;
	double x[SGP_NP], ff;
	for (int k = 0; k < SGP_NP; k++)
		x[k] = init[k];
	const int bad = sgp_lm<SGP_NP>(ev, x, &ff, &o.iters);
	double t = ff;
	for (int k = 0; k < SGP_NP; k++)
		t += x[k];
	if (bad || !sgp_finite(t)) {
		o.status = SG_FIT_NONFINITE;
		return;
	}
	sgp_finish(x, ff, ev.flux(x[0]), n, n2 / 2, cx, cy, norm, scale_x, scale_y, roundness, o);
}

/* a whole box sequentially: psf_global_minimisation(z, bg, layer, FALSE, FALSE), psf_update_units,
 * is_star and xpos / ypos of the candidate (cx, cy); box[i * 2r + j], r >= 1 */
static inline void sg_psf_fit_box(const uint16_t *box, int r, double bg, int cx, int cy, double norm, double scale_x,
		double scale_y, double roundness, double init[SGP_NP], SgPsfFit &o) {
	const int n2 = 2 * r;
	SgPsfSeqEval ev = {box, n2, n2};
	sgp_init_box(box, n2, n2, bg, [n2](const uint16_t *b, int i, int j) { return sgp_median3x3(b, n2, i, j); }, init);
	sgp_fit(ev, init, n2, cx, cy, norm, scale_x, scale_y, roundness, o);
}
