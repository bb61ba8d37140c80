/*
 * sg_ecc_step.h - the scalar part of one ECC iteration (include/sirilgpu.h, sg_register_ecc_u16*),
 * host + device: what findTransform_ECC (src/opencv/ecc/ecc.cpp:447-550) does, for
 * WARP_MODE_TRANSLATION, once its whole-image sums are known.  The iteration kernel of sg_ecc.hip
 * takes the sums as raw moments in one pass (SGE_* below); this header expands the masked means
 * out of them and keeps the float and double casts of the source: the Hessian entries, the
 * projections and the update are floats, everything else is double.  tests/ecc_ref.py
 * (step_moments) is the numpy restatement of this file, and tests/test_ecc_cpu.py holds the two
 * equal bit for bit (IEEE add, mul, div and sqrt, no contraction).
 *
 * Version-dependent OpenCV forms, fixed here as in tests/ecc_ref.py:
 *   - subtract(Mat32f, Scalar) converts the mean to float first: the expansions use (float)mean;
 *   - pow(norm(g), 2) is taken as r * r of r = sqrt(sum g^2);
 *   - invert() of a 2x2 float matrix: determinant and 1 / det in double, entries cast to float,
 *     all zero when the determinant is 0;
 *   - gemm of float matrices accumulates in double and casts the sum;
 *   - lambda * templateZM - imageWarped (addWeighted) takes lambda as a float.
 */
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define SGE_HD __host__ __device__ static inline
#else
#define SGE_HD static inline
#endif

#define SGE_MAX_ITER 50		/* number_of_iterations (ecc.cpp:562) */
#define SGE_EPS 0.001		/* termination_eps (:563) */

/* raw moments of one iteration: on the mask, off the mask, over all pixels */
enum {
	SGE_N = 0,		/* pixels on the mask */
	SGE_SI, SGE_SII,	/* on: sum iw, iw^2 */
	SGE_ST, SGE_STT,	/* on: sum t, t^2 */
	SGE_STI,		/* on: sum t iw */
	SGE_GXI, SGE_GYI,	/* on: sum gx iw, gy iw */
	SGE_GXT, SGE_GYT,	/* on: sum gx t, gy t */
	SGE_GX, SGE_GY,		/* on: sum gx, gy */
	SGE_OGXI, SGE_OGYI,	/* off: sum gx iw, gy iw (the warped image keeps its raw value there) */
	SGE_HXX, SGE_HXY, SGE_HYY,	/* all: sum gx^2, gx gy, gy^2 */
	SGE_NMOM
};

typedef struct {
	float tx, ty;		/* the map's translation column */
	double rho, last_rho;
	int32_t iter;		/* loop bodies run */
	int32_t done;
	int32_t failed;
	int32_t pad;
} sge_state;

SGE_HD void sge_state_init(sge_state *s) {
	s->tx = 0.f;
	s->ty = 0.f;
	s->rho = -1.0;
	s->last_rho = -SGE_EPS;
	s->iter = 0;
	s->done = 0;
	s->failed = 0;
	s->pad = 0;
}

SGE_HD int sge_finite(double x) {
	return x - x == 0.0;
}

/*
 * warpAffine's fixed-point coordinates for a pure translation t (AB_BITS 10, INTER_BITS 5): the
 * bilinear taps of output x are source ioff + x and ioff + x + 1 with the fraction frac / 32, the
 * nearest tap of the mask is source moff + x.  cvRound is round-half-even.  |t| beyond 2^20 pixels
 * (where the source overflows an int; unpinned) is held there: every tap is outside either way.
 */
SGE_HD void sge_offsets(float t, int *ioff, int *frac, int *moff) {
	double r = rint((double)t * 1024.0);
	if (r > 1073741824.0)
		r = 1073741824.0;
	if (r < -1073741824.0)
		r = -1073741824.0;
	const int ri = (int)r;
	const int o = (ri + 16) >> 5;
	*ioff = o >> 5;
	*frac = o & 31;
	*moff = (ri + 512) >> 10;
}

/* one loop body after its sums: m[SGE_NMOM] -> the next state */
SGE_HD void sge_step(const double *m, sge_state *s) {
	const double n = m[SGE_N];
	s->last_rho = s->rho;
	/* meanStdDev under the mask: double mean, variance sq / n - mean^2 held at 0 */
	const double mi = m[SGE_SI] / n, mt = m[SGE_ST] / n;
	double vi = m[SGE_SII] / n - mi * mi, vt = m[SGE_STT] / n - mt * mt;
	if (vi < 0.0)
		vi = 0.0;
	if (vt < 0.0)
		vt = 0.0;
	const double si = sqrt(vi), st = sqrt(vt);
	const double img_norm = sqrt(n * si * si), tmp_norm = sqrt(n * st * st);
	/* the zero-mean planes subtract the float mean */
	const double mif = (double)(float)mi, mtf = (double)(float)mt;
	const double corr = m[SGE_STI] - mtf * m[SGE_SI] - mif * m[SGE_ST] + n * mtf * mif;
	const double ipx = m[SGE_GXI] - mif * m[SGE_GX] + m[SGE_OGXI];
	const double ipy = m[SGE_GYI] - mif * m[SGE_GY] + m[SGE_OGYI];
	const double tpx = m[SGE_GXT] - mtf * m[SGE_GX];
	const double tpy = m[SGE_GYT] - mtf * m[SGE_GY];
	/* Hessian and its inverse */
	const double rx = sqrt(m[SGE_HXX]), ry = sqrt(m[SGE_HYY]);
	const float h00 = (float)(rx * rx), h01 = (float)m[SGE_HXY], h11 = (float)(ry * ry);
	const double det = (double)h00 * (double)h11 - (double)h01 * (double)h01;
	float i00 = 0.f, i01 = 0.f, i11 = 0.f;
	if (det != 0.0) {
		const double d = 1.0 / det;
		i00 = (float)((double)h11 * d);
		i11 = (float)((double)h00 * d);
		i01 = (float)(-(double)h01 * d);
	}
	double rho = corr / (img_norm * tmp_norm);
	const float ip0 = (float)ipx, ip1 = (float)ipy, tp0 = (float)tpx, tp1 = (float)tpy;
	const float iph0 = (float)((double)i00 * (double)ip0 + (double)i01 * (double)ip1);
	const float iph1 = (float)((double)i01 * (double)ip0 + (double)i11 * (double)ip1);
	const double lambda_n = img_norm * img_norm - ((double)ip0 * (double)iph0 + (double)ip1 * (double)iph1);
	const double lambda_d = corr - ((double)tp0 * (double)iph0 + (double)tp1 * (double)iph1);
	if (lambda_d <= 0.0)
		rho = -1.0;	/* and the loop goes on */
	const double lf = (double)(float)(lambda_n / lambda_d);
	const float ep0 = (float)(lf * tpx - ipx), ep1 = (float)(lf * tpy - ipy);
	const float dp0 = (float)((double)i00 * (double)ep0 + (double)i01 * (double)ep1);
	const float dp1 = (float)((double)i01 * (double)ep0 + (double)i11 * (double)ep1);
	s->tx = s->tx + dp0;
	s->ty = s->ty + dp1;
	s->rho = rho;
	s->iter++;
	if (!sge_finite(rho) || !sge_finite((double)s->tx) || !sge_finite((double)s->ty)) {
		s->done = 1;
		s->failed = 1;
	} else if (s->iter >= SGE_MAX_ITER || !(fabs(rho - s->last_rho) >= SGE_EPS)) {
		s->done = 1;
		s->failed = rho > 0.0 ? 0 : ((int)rho != 0);	/* findTransform returns (int)rho */
	}
}

/* what register_ecc stores for a finished frame (registration.c:870-890, utils.c:60-66) */
SGE_HD int sge_round_to_int(double x) {
	if (x > 2147483646.0)	/* the reference asserts here; held at the ends */
		return 2147483647;
	if (x < -2147483646.0)
		return -2147483647;
	if (x >= 0.0)
		return (int)(x + 0.5);
	return (int)(x - 0.5);
}

SGE_HD void sge_result(const sge_state *s, float *dx, float *dy, int *shiftx, int *shifty) {
	const int ok = !s->failed && s->rho > 0.0;	/* -1 < rho <= 0: success with the memset zeros */
	*dx = ok ? s->tx : 0.f;
	*dy = ok ? s->ty : 0.f;
	*shiftx = -sge_round_to_int((double)*dx);
	*shifty = -sge_round_to_int((double)*dy);
}
