/*
 * sg_prepro_plan.hpp - the host-only plan of a preprocessing sequence (include/sirilgpu.h,
 * sg_prepro_*): everything seqpreprocess (src/core/siril.c:1019-1169) decides once per sequence
 * or per frame on the host, with no HIP in it, so tests/test_prepro_cpu.py builds and checks it
 * without a GPU:
 *   - the flat's mean and the float level (statistics() -> FnMeanSigma_ushort, quantize.c:126-190);
 *   - the dark's sigma, histogram median and the hot / cold thresholds, the deviant list
 *     (find_deviant_pixels, cosmetic_correction.c:176-240);
 *   - the derived masters (flat with 0 -> 1, round_to_WORD(dark - offset) for the dark fit);
 *   - the schedule that makes the in-place, in-order correction parallel (sgp_build_schedule);
 *   - the golden-section bookkeeping (SgGolden) and the row-median finish of the noise
 *     (sgp_noise_finish), plus host forms of one noise row and one corrected pixel, which are the
 *     check of the kernels' forms (sg_prepro.hip).
 */
#pragma once
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <algorithm>
#include <vector>
#include "../../include/sirilgpu.h"

/* shared by the host plan and the kernels */
#if defined(__HIPCC__)
#define SGP_HD __host__ __device__ static inline
#else
#define SGP_HD static inline
#endif

#define SGP_COLD 0x80000000u	/* list / item entries: pixel index | SGP_COLD for a cold pixel */

/* round_to_WORD, src/core/utils.c:68-74 */
SGP_HD uint16_t sgp_rtw(double x) {
	if (x <= 0.0)
		return 0;
	if (x > 65535.0)
		return 65535;
	return (uint16_t)(x + 0.5);
}

/* FnMeanSigma_ushort with nullcheck, null value 0: the sums run sequentially in double (sum2 can
 * pass 2^53 on a large image, where the rounding order shows) */
static inline void sgp_mean_sigma_u16(const uint16_t *a, int64_t npix, int64_t *ngood, double *mean, double *sigma) {
	int64_t n = 0;
	double sum = 0., sum2 = 0., xtemp;
	for (int64_t i = 0; i < npix; i++)
		if (a[i] != 0) {
			n++;
			xtemp = (double)a[i];
			sum += xtemp;
			sum2 += (xtemp * xtemp);
		}
	*ngood = n;
	if (n > 1) {
		xtemp = sum / n;
		*mean = xtemp;
		*sigma = sqrt((sum2 / n) - (xtemp * xtemp));
	} else if (n == 1) {
		*mean = sum;
		*sigma = 0.0;
	} else {
		*mean = 0.;
		*sigma = 0.;
	}
}

/* FnMeanSigma_int without nullcheck from exact integer sums (|sum| and sum2 stay below 2^53 for a
 * row of at most 65535 differences of WORDs, so the reference's double sums are these integers) */
SGP_HD void sgp_mean_sigma_sums(int64_t n, int64_t sum, int64_t sum2, double *mean, double *sigma) {
	if (n > 1) {
		const double xtemp = (double)sum / (double)n;
		*mean = xtemp;
		*sigma = sqrt(((double)sum2 / (double)n) - (xtemp * xtemp));
	} else if (n == 1) {
		*mean = (double)sum;
		*sigma = 0.0;
	} else {
		*mean = 0.;
		*sigma = 0.;
	}
}

/* siril_stats_ushort_median (statistics.c:47-63) on computeHisto's histogram (histogram.c:111-127):
 * 65536 uniform bins over [0, 65535), so 65535 itself is not counted; from bin 1, the first bin
 * whose running count exceeds ngood * 0.5, else 0 */
static inline double sgp_hist_median(const uint16_t *a, int64_t npix, int64_t ngood) {
	std::vector<int64_t> h(65536, 0);
	for (int64_t i = 0; i < npix; i++)
		if (a[i] < 65535)
			h[a[i]]++;
	double sum = 0.0;
	for (int i = 1; i < 65536; i++) {
		sum += (double)h[i];
		if (sum > ((double)ngood * 0.5))
			return (double)i;
	}
	return 0.0;
}

/* one pixel of cosmeticCorrection: getAverage3x3 (hot) / getMedian5x5 (cold) at (x, y) of buf.
 * Cold: the reference's zero-padded, sorted array of 24 read at [23 - n, 22] is the multiset
 * {0} with the n - 1 smallest neighbours (n = 24 reads value[-1], taken as 0: sirilgpu.h) */
static inline uint16_t sgp_correct_one(const uint16_t *buf, int W, int H, int x, int y, int cold, int is_cfa) {
	const int step = is_cfa ? 2 : 1, rad = cold ? 2 * step : step;
	uint16_t v[25];
	int n = 0;
	double value = 0;
	for (int yy = y - rad; yy <= y + rad; yy += step)
		for (int xx = x - rad; xx <= x + rad; xx += step)
			if (yy >= 0 && yy < H && xx >= 0 && xx < W && (xx != x || yy != y)) {
				v[n++] = buf[xx + (int64_t)yy * W];
				value += (double)buf[xx + (int64_t)yy * W];
			}
	if (n == 0)
		return 0;
	if (!cold)
		return sgp_rtw(value / n);
	std::sort(v, v + n);
	const int i0 = (n - 1) / 2, i1 = n / 2;	/* positions in {0, v[0], ..., v[n - 2]} */
	const double m0 = i0 == 0 ? 0.0 : (double)v[i0 - 1], m1 = i1 == 0 ? 0.0 : (double)v[i1 - 1];
	return sgp_rtw(n & 1 ? m0 : (m0 + m1) / 2.0);
}

/* one row of FnNoise1_ushort on p = max(raw - round_to_WORD(dark * k), 0) (imoper SUB after soper
 * MUL), null value 0: returns 1 and the row's final stdev when the row contributes */
static inline int sgp_noise_row(const uint16_t *raw, const uint16_t *dark, int W, double k, double *sd_out) {
	std::vector<int> d;
	int v1 = 0;
	for (int x = 0; x < W; x++) {
		const int dk = sgp_rtw((double)dark[x] * k);
		const int p = raw[x] > dk ? raw[x] - dk : 0;
		if (!p)
			continue;
		if (v1)
			d.push_back(v1 - p);
		v1 = p;
	}
	if (d.size() < 2)
		return 0;
	double mean[4], sd[4];
	int np = 0;	/* clip conditions in force */
	int64_t nvals = 0, s = 0, s2 = 0;
	for (int di : d) {
		nvals++;
		s += di;
		s2 += (int64_t)di * di;
	}
	sgp_mean_sigma_sums(nvals, s, s2, &mean[0], &sd[0]);
	if (sd[0] > 0.)
		for (int iter = 0; iter < 3; iter++) {
			np = iter + 1;
			int64_t kk = 0;
			s = s2 = 0;
			for (int di : d) {
				bool keep = true;
				for (int j = 0; j < np; j++)	/* the kept sets are nested */
					keep = keep && fabs((double)di - mean[j]) < 5. * sd[j];
				if (keep) {
					kk++;
					s += di;
					s2 += (int64_t)di * di;
				}
			}
			if (kk == nvals) {
				mean[np] = mean[iter];
				sd[np] = sd[iter];
				break;
			}
			nvals = kk;
			sgp_mean_sigma_sums(nvals, s, s2, &mean[np], &sd[np]);
		}
	*sd_out = sd[np];
	return 1;
}

/* the image value of FnNoise1_ushort from the contributing rows' values (quantize.c:767-777) */
static inline double sgp_noise_finish(const double *sd, const int *contributed, int H, int W) {
	if (W < 3)
		return 0.0;
	std::vector<double> diffs;
	for (int y = 0; y < H; y++)
		if (contributed[y])
			diffs.push_back(sd[y]);
	const size_t nrows = diffs.size();
	double xnoise;
	if (nrows == 0)
		xnoise = 0;
	else if (nrows == 1)
		xnoise = diffs[0];
	else {
		/* the two middle order statistics of the reference's qsort, by selection */
		const size_t lo = (nrows - 1) / 2, hi = nrows / 2;
		std::nth_element(diffs.begin(), diffs.begin() + lo, diffs.end());
		const double a = diffs[lo], b = hi == lo ? a : *std::min_element(diffs.begin() + hi, diffs.end());
		xnoise = (a + b) / 2.;
	}
	return .70710678 * xnoise;
}

/* goldenSectionSearch (siril.c:922-943) as a state machine fed with objective values: want()
 * names the points still to evaluate (both at the start, then only the new one: the objective is
 * deterministic, so the point carried over keeps its value), feed() takes their values in that
 * order and advances one iteration */
struct SgGolden {
	double a = 0, b = 0, c = 0, d = 0, fc = 0, fd = 0, tol = 0, gr = 0;
	int have_c = 0, have_d = 0, done = 0, iters = 0;
	void init(double lo, double up, double tolerance) {
		gr = (sqrt(5) - 1) / 2;
		a = lo;
		b = up;
		tol = tolerance;
		c = b - gr * (b - a);
		d = a + gr * (b - a);
		have_c = have_d = done = iters = 0;
	}
	int want(double k[2]) const {
		int n = 0;
		if (done)
			return 0;
		if (!have_c)
			k[n++] = c;
		if (!have_d)
			k[n++] = d;
		return n;
	}
	void feed(const double *f) {
		int n = 0;
		if (done)
			return;
		if (!have_c)
			fc = f[n++];
		if (!have_d)
			fd = f[n++];
		have_c = have_d = 1;
		if (fc < fd) {
			b = d;
			d = c;
			fd = fc;
			c = b - gr * (b - a);
			have_c = 0;
		} else {
			a = c;
			c = d;
			fc = fd;
			d = a + gr * (b - a);
			have_d = 0;
		}
		iters++;
		if (!(fabs(c - d) > tol))
			done = 1;
	}
	double result() const { return ((b + a) / 2); }
};

struct SgPreproPlan {
	int W = 0, H = 0, C = 0;
	int use_offset = 0, use_dark = 0, use_flat = 0, optd = 0, cosme_applies = 0, is_cfa = 0;
	float level = 0.f;
	double flat_mean = 0.;
	int64_t dark_ngood = 0, icold = 0, ihot = 0;
	double dark_sigma = 0., dark_median = 0., thres_cold = 0., thres_hot = 0.;
	std::vector<uint16_t> flat1;	/* [C][H][W]: the flat with 0 -> 1 (fdiv :266-267) */
	std::vector<uint16_t> darkfit;	/* [H][W]: round_to_WORD(dark - offset) (darkOptimization :977-978), optd with an offset */
	std::vector<uint32_t> list;	/* deviant pixels in the reference's (raster) order */
	std::vector<uint32_t> items;	/* the same entries grouped by component, list order inside each */
	std::vector<uint32_t> comp_start;	/* [components + 1] into items */
	uint32_t longest = 0;
	char err[256] = "";
};

/*
 * The schedule.  Correcting deviant pixel i reads its window; a deviant pixel j in that window
 * must already be corrected if it precedes i in the list and must still be uncorrected if it
 * follows i.  Both orders bind i and j, so pixels are joined whenever one lies in the other's
 * window, and the connected components of that relation are independent of each other: walking
 * every component in list order gives the sequential loop's result for any list, whatever runs
 * between components (and frames) in parallel.
 */
static inline void sgp_build_schedule(SgPreproPlan &p) {
	const size_t n = p.list.size();
	p.items.clear();
	p.comp_start.assign(1, 0);
	p.longest = 0;
	if (!n)
		return;
	const int W = p.W, H = p.H, step = p.is_cfa ? 2 : 1;
	std::vector<uint8_t> tmap((size_t)W * H, 0);
	for (uint32_t e : p.list)
		tmap[e & ~SGP_COLD] = 1;
	std::vector<uint32_t> parent(n);
	for (size_t i = 0; i < n; i++)
		parent[i] = (uint32_t)i;
	auto find = [&](uint32_t i) {
		while (parent[i] != i) {
			parent[i] = parent[parent[i]];
			i = parent[i];
		}
		return i;
	};
	auto index_of = [&](uint32_t pix) {	/* the list is sorted by pixel index */
		size_t lo = 0, hi = n;
		while (lo < hi) {
			const size_t mid = (lo + hi) / 2;
			if ((p.list[mid] & ~SGP_COLD) < pix)
				lo = mid + 1;
			else
				hi = mid;
		}
		return (uint32_t)lo;
	};
	for (size_t i = 0; i < n; i++) {
		const uint32_t pix = p.list[i] & ~SGP_COLD;
		const int x = (int)(pix % (uint32_t)W), y = (int)(pix / (uint32_t)W);
		const int rad = (p.list[i] & SGP_COLD) ? 2 * step : step;
		for (int yy = y - rad; yy <= y + rad; yy += step)
			for (int xx = x - rad; xx <= x + rad; xx += step) {
				if (yy < 0 || yy >= H || xx < 0 || xx >= W || (xx == x && yy == y))
					continue;
				const uint32_t q = (uint32_t)yy * (uint32_t)W + (uint32_t)xx;
				if (!tmap[q])
					continue;
				const uint32_t ra = find((uint32_t)i), rb = find(index_of(q));
				if (ra != rb)
					parent[ra > rb ? ra : rb] = ra > rb ? rb : ra;
			}
	}
	/* components numbered by their first pixel; items in list order inside each */
	std::vector<uint32_t> comp(n), count;
	for (size_t i = 0; i < n; i++) {
		const uint32_t r = find((uint32_t)i);
		if (r == i) {
			comp[i] = (uint32_t)count.size();
			count.push_back(0);
		} else
			comp[i] = comp[r];	/* the root is the smallest index of its set: already numbered */
		count[comp[i]]++;
	}
	p.comp_start.assign(count.size() + 1, 0);
	for (size_t c = 0; c < count.size(); c++) {
		p.comp_start[c + 1] = p.comp_start[c] + count[c];
		p.longest = std::max(p.longest, count[c]);
	}
	std::vector<uint32_t> fill(p.comp_start.begin(), p.comp_start.end() - 1);
	p.items.resize(n);
	for (size_t i = 0; i < n; i++)
		p.items[fill[comp[i]]++] = p.list[i];
}

static inline int sgp_fail(SgPreproPlan &p, int code, const char *msg) {
	snprintf(p.err, sizeof p.err, "%s", msg);
	return code;
}

/* everything seqpreprocess decides before its frame loop */
static inline int sg_prepro_plan(const sg_prepro_desc *d, SgPreproPlan &p) {
	p = SgPreproPlan();
	if (!d)
		return sgp_fail(p, SG_ERR_GENERIC, "no descriptor");
	if (d->width <= 0 || d->height <= 0 || d->nb_layers <= 0)
		return sgp_fail(p, SG_ERR_SIZE, "preprocessing: width, height and nb_layers must be positive");
	if ((int64_t)d->width * d->height >= (1ll << 31))
		return sgp_fail(p, SG_ERR_SIZE, "preprocessing: a plane of 2^31 pixels or more");
	if (d->nb_layers > 3)
		return sgp_fail(p, SG_ERR_GENERIC, "preprocessing: more than 3 layers");
	if (d->dark_optimization && !d->dark)
		return sgp_fail(p, SG_ERR_GENERIC, "dark optimization needs a master dark");
	if (d->dark_optimization && d->nb_layers != 1)
		return sgp_fail(p, SG_ERR_GENERIC, "dark optimization is refused for nb_layers != 1 (the reference "
				"indexes layers 1 and 2 of a one-layer copy)");
	if (d->cosmetic && !d->dark)
		return sgp_fail(p, SG_ERR_GENERIC, "cosmetic correction needs a master dark");
	p.W = d->width;
	p.H = d->height;
	p.C = d->nb_layers;
	p.use_offset = d->offset != nullptr;
	p.use_dark = d->dark != nullptr;
	p.use_flat = d->flat != nullptr;
	p.optd = d->dark_optimization != 0;
	p.is_cfa = d->is_cfa != 0;
	const int64_t npix = (int64_t)p.W * p.H;
	p.level = d->normalisation;
	if (p.use_flat) {
		if (d->autolevel) {
			int64_t ngood;
			double sigma;
			sgp_mean_sigma_u16(d->flat, npix, &ngood, &p.flat_mean, &sigma);
			if (ngood == 0)
				return sgp_fail(p, SG_ERR_GENERIC, "autolevel: the flat has no non-zero pixel (no statistics)");
			p.level = (float)p.flat_mean;	/* args->normalisation is a float */
		}
		p.flat1.assign(d->flat, d->flat + npix * p.C);
		for (uint16_t &f : p.flat1)
			if (f == 0)
				f = 1;
	}
	if (p.optd && p.use_offset) {
		p.darkfit.resize(npix);
		for (int64_t i = 0; i < npix; i++)
			p.darkfit[i] = sgp_rtw((double)((int)d->dark[i] - (int)d->offset[i]));
	}
	p.cosme_applies = d->cosmetic && p.use_dark && p.C == 1;
	if (p.cosme_applies) {
		double mean;
		sgp_mean_sigma_u16(d->dark, npix, &p.dark_ngood, &mean, &p.dark_sigma);
		if (p.dark_ngood == 0) {	/* statistics() returns NULL: find_deviant_pixels gives no list */
			sgp_build_schedule(p);
			return SG_OK;
		}
		p.dark_median = sgp_hist_median(d->dark, npix, p.dark_ngood);
		if (d->cosme_sigma[0] == -1.0)
			p.thres_cold = -1.0;
		else {
			const double val = p.dark_median - (d->cosme_sigma[0] * p.dark_sigma);
			p.thres_cold = (val > 0) ? val : 0.0;
		}
		if (d->cosme_sigma[1] == -1.0)
			p.thres_hot = 65535.0 + 1;
		else {
			const double val = p.dark_median + (d->cosme_sigma[1] * p.dark_sigma);
			p.thres_hot = (val > 65535.0) ? 65535.0 : val;
		}
		for (int64_t i = 0; i < npix; i++) {
			const double pixel = (double)d->dark[i];
			if (pixel >= p.thres_hot) {
				p.list.push_back((uint32_t)i);
				p.ihot++;
			} else if (pixel <= p.thres_cold) {
				p.list.push_back((uint32_t)i | SGP_COLD);
				p.icold++;
			}
		}
		sgp_build_schedule(p);
	}
	return SG_OK;
}
