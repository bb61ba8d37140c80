/*
 * sg_ikss.h - the IKSS location / scale of one frame from its prefix-count table
 * (statistics.c IKSS :152-187 with siril_stats_double_mad :82-100 and
 * siril_stats_double_bwmv :128-150), host + device.
 *
 * The reference sorts the frame's non-zero samples as doubles x / norm and iterates median,
 * MAD (a second sort), biweight midvariance (sequential double sums over the sorted data)
 * and 4-sigma clipping.  Here all of it reads P[x * nf + f] = #samples of frame f below x
 * (x = 0..65536, zeros not counted; row 65536 = the total): medians are rank lookups, the
 * MAD is a merge of the two monotone delta sequences on either side of the median, the
 * BWMV sums add each distinct value's term count(x) times with sg_add_repeat (sg_repadd.h),
 * and the clipping loops are binary searches.  Every double expression is written as the
 * reference writes it and must not be contracted (-ffp-contract=off).
 *
 * k_ikss_solve (sg_stats.hip) calls sg_ikss_frame with one lane per frame.  The same source
 * built for the host is compared bit for bit with the sort-based CPU restatement of
 * statistics() on random sample sets by tests/test_ikss_cpu.py.
 */
#ifndef SG_IKSS_H
#define SG_IKSS_H

#include <stddef.h>
#include <stdint.h>
#include <math.h>
#include "sg_repadd.h"

#if defined(__HIPCC__)
#define SG_IK_HD __host__ __device__ static inline
#else
#define SG_IK_HD static inline
#endif

#define SG_IK_BINS 65536

struct SgIk {
	const uint32_t *P;
	int nf, f;
	double norm;
};

SG_IK_HD uint32_t ik_P(const SgIk &k, int x) {
	return k.P[(size_t)x * k.nf + k.f];
}
SG_IK_HD double ik_val(const SgIk &k, int x) {
	return (double)x / k.norm;	/* newdata[i] = (double) data[i] / ((double) hist_size - 1) (:281) */
}
/* value of the sample at rank r (0-based, sorted non-zero samples) */
SG_IK_HD int ik_x_at(const SgIk &k, uint32_t r) {
	int lo = 1, hi = SG_IK_BINS - 1;
	while (lo < hi) {
		const int mid = (lo + hi) >> 1;
		if (ik_P(k, mid + 1) > r)
			hi = mid;
		else
			lo = mid + 1;
	}
	return lo;
}
/* samples of value x among ranks [i, j) */
SG_IK_HD uint32_t ik_cnt(const SgIk &k, int x, uint32_t i, uint32_t j) {
	uint32_t a = ik_P(k, x), b = ik_P(k, x + 1);
	a = a > i ? a : i;
	b = b < j ? b : j;
	return b > a ? b - a : 0u;
}
/* gsl_stats_median_from_sorted_data(data + i, 1, j - i) */
SG_IK_HD double ik_median(const SgIk &k, uint32_t i, uint32_t j) {
	const uint32_t n = j - i, lhs = i + (n - 1) / 2, rhs = i + n / 2;
	const double a = ik_val(k, ik_x_at(k, lhs));
	if (lhs == rhs)
		return a;
	return (a + ik_val(k, ik_x_at(k, rhs))) / 2.0;
}
/* siril_stats_double_mad (:82-100): median of |data - m| over ranks [i, j) */
SG_IK_HD double ik_mad(const SgIk &k, uint32_t i, uint32_t j, double m) {
	const uint32_t n = j - i, rl = (n - 1) / 2, rr = n / 2;
	const int xi = ik_x_at(k, i), xj = ik_x_at(k, j - 1);
	int lo_b = xi, hi_b = xj + 1;	/* first x with val(x) >= m */
	while (lo_b < hi_b) {
		const int mid = (lo_b + hi_b) >> 1;
		if (ik_val(k, mid) >= m)
			hi_b = mid;
		else
			lo_b = mid + 1;
	}
	int hi = lo_b, lo = lo_b - 1;
	uint32_t seen = 0;
	double vl = 0.0, vr = 0.0;
	bool have_l = false;
	for (;;) {
		while (lo >= xi && ik_cnt(k, lo, i, j) == 0)
			lo--;
		while (hi <= xj && ik_cnt(k, hi, i, j) == 0)
			hi++;
		bool take_hi;
		if (lo < xi)
			take_hi = true;
		else if (hi > xj)
			take_hi = false;
		else
			take_hi = fabs(ik_val(k, hi) - m) <= fabs(ik_val(k, lo) - m);
		const int x = take_hi ? hi : lo;
		const double d = fabs(ik_val(k, x) - m);
		const uint32_t c = ik_cnt(k, x, i, j);
		if (!have_l && rl < seen + c) {
			vl = d;
			have_l = true;
		}
		if (rr < seen + c) {
			vr = d;
			break;
		}
		seen += c;
		if (take_hi)
			hi++;
		else
			lo--;
	}
	return rl == rr ? vl : (vl + vr) / 2.0;
}
/* siril_stats_double_bwmv (:128-150) over the sorted ranks [i, j) */
SG_IK_HD double ik_bwmv(const SgIk &k, uint32_t i, uint32_t j, double mad, double median) {
	double bwmv = 0.0, up = 0.0, down = 0.0;
	if (mad > 0.0) {
		const int xi = ik_x_at(k, i), xj = ik_x_at(k, j - 1);
		for (int x = xi; x <= xj; x++) {
			const uint32_t c = ik_cnt(k, x, i, j);
			if (!c)
				continue;
			const double d = ik_val(k, x);
			const double yi = (d - median) / (9 * mad);
			const double yi2 = yi * yi;
			const double ai = (fabs(yi) < 1.0) ? 1.0 : 0.0;
			const double tu = ai * ((d - median) * (d - median)) * (((1 - yi2) * (1 - yi2)) * ((1 - yi2) * (1 - yi2)));
			const double td = (ai * (1 - yi2) * (1 - 5 * yi2));
			up = sg_add_repeat(up, tu, c);
			down = sg_add_repeat(down, td, c);
		}
		bwmv = (double)(j - i) * (up / (down * down));
	}
	return bwmv;
}

/* IKSS (:152-187) of frame f of the prefix table P[SG_IK_BINS + 1][nf]; maxi = the frame's
 * maximum over all layers (norm = 255 or 65535: get_normalized_value, src/core/utils.c:454-459).
 * Location / scale come back in the original range (:286-288).  Returns 0, -1 when the frame
 * has no non-zero sample (ngoodpix == 0: statistics() returns NULL, :249-252) or -2 when the
 * loop did not converge (the reference would not return). */
SG_IK_HD int sg_ikss_frame(const uint32_t *P, int nf, int f, uint32_t maxi, double *location_out, double *scale_out) {
	SgIk k;
	k.P = P;
	k.nf = nf;
	k.f = f;
	k.norm = maxi <= 255u ? 255.0 : 65535.0;
	const uint32_t n = ik_P(k, SG_IK_BINS);
	double location = 0.0, scale = 0.0;
	int r = 0;
	if (!n) {
		r = -1;
	} else {
		uint32_t i = 0, j = n;
		double s0 = 1;
		for (int guard = 0;; guard++) {
			if (guard > 10000) {
				r = -2;
				break;
			}
			if (j - i < 1) {
				location = scale = 0;
				break;
			}
			const double m = ik_median(k, i, j);
			const double mad = ik_mad(k, i, j, m);
			const double s = sqrt(ik_bwmv(k, i, j, mad, m));
			if (s < 2E-23) {
				location = m;
				scale = 0;
				break;
			}
			if (((s0 - s) / s) < 10E-6) {
				location = m;
				scale = 0.991 * s;
				break;
			}
			s0 = s;
			const double xlow = m - 4 * s, xhigh = m + 4 * s;
			/* while (data[i] < xlow) i++: first x with val(x) >= xlow */
			int lo = 1, hi = SG_IK_BINS;
			while (lo < hi) {
				const int mid = (lo + hi) >> 1;
				if (ik_val(k, mid) >= xlow)
					hi = mid;
				else
					lo = mid + 1;
			}
			const uint32_t ni = ik_P(k, lo);
			i = ni > i ? ni : i;
			/* while (data[j - 1] > xhigh) j--: last x with val(x) <= xhigh */
			lo = 0;
			hi = SG_IK_BINS - 1;
			while (lo < hi) {
				const int mid = (lo + hi + 1) >> 1;
				if (ik_val(k, mid) <= xhigh)
					lo = mid;
				else
					hi = mid - 1;
			}
			const uint32_t nj = ik_P(k, lo + 1);
			j = nj < j ? nj : j;
		}
	}
	*location_out = location * k.norm;
	*scale_out = scale * k.norm;
	return r;
}

#endif /* SG_IKSS_H */
