/*
 * sg_cosme.h - the per-pixel rule of the automatic cosmetic correction (include/sirilgpu.h,
 * sg_cosme_autodetect*), host + device: autoDetect (src/algos/cosmetic_correction.c:384-435) with
 * getAverage3x3 (:102-126) and getMedian5x5 (:34-67), and the finish of the two statistics it
 * takes from statistics() (src/algos/statistics.c:207-326).  The kernels of sg_cosme.hip and the
 * host programs of tests/test_cosme_cpu.py are written in these functions; tests/cosme_ref.py is
 * the numpy restatement.  Every double expression is written as the reference writes it and must
 * be compiled without contraction.
 *
 * The neighbourhoods are read through a getter `g.at(x, y)`, called with in-frame coordinates
 * only: the LDS tile of the main pass (SgcTileGet), or the frame together with the sparse record
 * of the pixels corrected so far (SgcStateGet) in the rounds that resolve the scan-order
 * dependence.
 */
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define SGC_HD __host__ __device__ static inline
#define SGC_HD_MEMBER __host__ __device__ inline
#else
#define SGC_HD static inline
#define SGC_HD_MEMBER inline
#endif
/* a kind-bit word another thread of the same round may be updating */
#define SGC_LOAD_BITS(p) __atomic_load_n((p), __ATOMIC_RELAXED)

enum { SGC_NONE = 0, SGC_HOT = 1, SGC_COLD = 2 };

/* round_to_WORD, src/core/utils.c:68-74 */
SGC_HD uint32_t sgc_rtw(double x) {
	if (x <= 0.0)
		return 0;
	if (x > 65535.0)
		return 65535;
	return (uint32_t)(uint16_t)(x + 0.5);
}

/*
 * One layer's rule.  The three tests of a pixel that need no neighbour, and the test of the 3x3
 * average, compare an integer with a double that is fixed per layer, so each is an integer
 * threshold:
 *   pixel > bkg + avgDev        <=>  pixel >= hot_min
 *   a < bkg + avgDev / 2        <=>  a <= a_max
 *   pixel + avgDev * sig[0] < bkg  <=>  pixel <= cold_max   (the left side is monotone in pixel)
 * A pixel's own value is the original one when the scan reaches it, so pixel < hot_min and
 * pixel > cold_max can never be corrected whatever happens to its neighbours.
 */
typedef struct {
	int64_t ngood;		/* 0: statistics() returns NULL, the frame fails at this layer */
	double bkg, avg_dev;
	double k3;		/* sig[1] * avgDev */
	double kc;		/* avgDev * sig[0] */
	double f0, f1;		/* amount, 1 - amount */
	int32_t hot_min;	/* 65536: never (or sig[1] == -1) */
	int32_t a_max;
	int32_t cold_max;	/* -1: never (or sig[0] == -1) */
	int32_t step;		/* 2 with is_cfa */
} sgc_rule;

/* from the layer's histogram sums: ngood, the histogram median and the exact sum |v - bkg| */
SGC_HD void sgc_rule_make(sgc_rule *r, int64_t ngood, uint32_t median, uint64_t sumabs, double sig0, double sig1,
		double amount, int is_cfa) {
	r->ngood = ngood;
	r->bkg = (double)median;
	r->avg_dev = ngood > 0 ? (double)sumabs / (double)ngood : 0.0;	/* gsl_stats_ushort_absdev_m */
	const double f0 = amount;
	r->f0 = f0;
	r->f1 = 1 - f0;
	r->step = is_cfa ? 2 : 1;
	r->hot_min = 65536;
	r->a_max = -1;
	r->cold_max = -1;
	r->k3 = 0.0;
	r->kc = 0.0;
	if (ngood <= 0)
		return;
	if (sig1 != -1.0) {
		const double k1 = r->avg_dev;
		const double k2 = k1 / 2;
		r->k3 = sig1 * k1;
		const double t1 = r->bkg + k1, t2 = r->bkg + k2;	/* both in [0, 131070] */
		r->hot_min = t1 >= 65535.0 ? 65536 : (int32_t)floor(t1) + 1;
		r->a_max = (int32_t)ceil(t2) - 1;
		if (r->a_max > 65535)
			r->a_max = 65535;
	}
	if (sig0 != -1.0) {
		const double k = r->avg_dev * sig0;
		r->kc = k;
		int lo = -1, hi = 65535;	/* the largest pixel with pixel + k < bkg */
		while (lo < hi) {
			const int mid = lo + (hi - lo + 1) / 2;
			if (((double)mid + k) < r->bkg)
				lo = mid;
			else
				hi = mid - 1;
		}
		r->cold_max = lo;
	}
}

/* getAverage3x3 (:102-126): the sum of WORDs is exact in double, so it is taken in integers; with
 * all 8 neighbours the divide by 8 and the + 0.5 are exact too.  No neighbour at all (a CFA plane
 * of at most 3 x 3 has such pixels; the reference divides 0 by 0 and converts the NaN): 0, as
 * sgp_hot_px. */
template <class G> SGC_HD uint32_t sgc_average(const G &g, int W, int H, int x, int y, int step) {
	uint32_t sum = 0;
	int n = 0;
#pragma unroll
	for (int dy = -1; dy <= 1; dy++)
#pragma unroll
		for (int dx = -1; dx <= 1; dx++) {
			if (dx == 0 && dy == 0)
				continue;
			const int xx = x + dx * step, yy = y + dy * step;
			if (yy >= 0 && yy < H && xx >= 0 && xx < W) {
				sum += g.at(xx, yy);
				n++;
			}
		}
	if (n == 8)
		return (sum + 4u) >> 3;
	return n ? sgc_rtw((double)sum / n) : 0u;
}

#define SGC_CSWAP(a, b)                          \
	do {                                     \
		const uint32_t _lo = a < b ? a : b; \
		const uint32_t _hi = a < b ? b : a; \
		a = _lo;                         \
		b = _hi;                         \
	} while (0)

/* getMedian5x5 (:34-67) with its start = 24 - n - 1: the median of one padding zero and the n - 1
 * smallest of the n in-frame neighbours.  The 24 values (outside the frame: above every WORD) are
 * sorted by Batcher's odd-even merge network for 32 (191 compare-exchanges, all indices constant),
 * then the two order statistics are picked by constant-index selects. */
template <class G> SGC_HD uint32_t sgc_median(const G &g, int W, int H, int x, int y, int step) {
	uint32_t v[32];
	int n = 0;
#pragma unroll
	for (int i = 0; i < 25; i++) {
		if (i == 12)
			continue;
		const int xx = x + (i % 5 - 2) * step, yy = y + (i / 5 - 2) * step;
		const bool in = yy >= 0 && yy < H && xx >= 0 && xx < W;
		v[i < 12 ? i : i - 1] = in ? g.at(xx, yy) : 0x10000u;
		n += in;
	}
#pragma unroll
	for (int i = 24; i < 32; i++)
		v[i] = 0x10000u;
	if (n == 0)
		return 0u;
#pragma unroll
	for (int p = 1; p < 32; p <<= 1)
#pragma unroll
		for (int k = p; k >= 1; k >>= 1)
#pragma unroll
			for (int j = k % p; j + k < 32; j += 2 * k)
#pragma unroll
				for (int i = 0; i < k; i++)
					if ((i + j) / (2 * p) == (i + j + k) / (2 * p) && i + j + k < 32)
						SGC_CSWAP(v[i + j], v[i + j + k]);
	const int r0 = (n - 1) / 2 - 1, r1 = n / 2 - 1;	/* ranks among the neighbours; -1: the zero */
	uint32_t m0 = 0, m1 = 0;
#pragma unroll
	for (int i = 0; i < 12; i++) {	/* n <= 24: r0 <= 10, r1 <= 11 */
		m0 = i == r0 ? v[i] : m0;
		m1 = i == r1 ? v[i] : m1;
	}
	return sgc_rtw((n & 1) ? (double)m0 : ((double)m0 + (double)m1) / 2.0);
}

/* the tests of a pixel that need no neighbour: SGC_HOT / SGC_COLD = worth a look, SGC_NONE = never
 * corrected */
SGC_HD int sgc_own(const sgc_rule &r, uint32_t pixel) {
	if ((int32_t)pixel >= r.hot_min)
		return SGC_HOT;
	if ((int32_t)pixel <= r.cold_max)
		return SGC_COLD;
	return SGC_NONE;
}

/*
 * A cheap necessary condition of the hot test's third part, pixel > m + k3, without the median:
 * m >= m0, the lower of the two order statistics, so at least r0 + 1 neighbours must themselves
 * satisfy pixel > v + k3.  v + k3 > pixel + 1 in exact arithmetic rules that out whatever the
 * rounding, so v <= floor(pixel - k3) + 2 is a superset; counting it takes 24 integer compares.
 */
template <class G> SGC_HD bool sgc_hot_maybe(const G &g, int W, int H, int x, int y, const sgc_rule &r, uint32_t pixel) {
	const double lim = floor((double)pixel - r.k3) + 2.0;
	if (lim < 0.0)
		return false;
	const uint32_t vmax = lim > 65535.0 ? 65535u : (uint32_t)lim;
	int n = 0, below = 0;
#pragma unroll
	for (int i = 0; i < 25; i++) {
		if (i == 12)
			continue;
		const int xx = x + (i % 5 - 2) * r.step, yy = y + (i / 5 - 2) * r.step;
		if (yy >= 0 && yy < H && xx >= 0 && xx < W) {
			n++;
			below += g.at(xx, yy) <= vmax;
		}
	}
	return below >= (n - 1) / 2;	/* r0 + 1 of them; r0 = -1: the zero, 0 <= vmax */
}

/* autoDetect's loop body (:409-431) for one pixel whose own tests say `own`: SGC_NONE, or the kind
 * of the hit and the value written, a * f0 + pixel * f1 or m * f0 + pixel * f1 in double as
 * written, truncated to WORD.  The hot and the cold test cannot both hold for sig >= 0 (hot needs
 * pixel > bkg, cold pixel < bkg), so at most one store happens. */
template <class G>
SGC_HD int sgc_decide(const G &g, int W, int H, int x, int y, const sgc_rule &r, uint32_t pixel, int own, uint16_t *val) {
	if (own == SGC_HOT) {
		const uint32_t a = sgc_average(g, W, H, x, y, r.step);
		if ((int32_t)a > r.a_max)
			return SGC_NONE;
		const uint32_t m = sgc_median(g, W, H, x, y, r.step);
		if (!((double)pixel > (double)m + r.k3))
			return SGC_NONE;
		*val = (uint16_t)((double)a * r.f0 + (double)pixel * r.f1);
		return SGC_HOT;
	}
	if (own == SGC_COLD) {
		const uint32_t m = sgc_median(g, W, H, x, y, r.step);
		if (!(((double)pixel + r.kc) < (double)m))
			return SGC_NONE;
		*val = (uint16_t)((double)m * r.f0 + (double)pixel * r.f1);
		return SGC_COLD;
	}
	return SGC_NONE;
}

/* ------------------------------------------------------------------ the main pass's tile */

#define SGC_TILE_W 64		/* output tile: 256 threads, a thread walks 8 rows of its column */
#define SGC_TILE_H 32
#define SGC_ROWS 8
#define SGC_THREADS (SGC_TILE_W * (SGC_TILE_H / SGC_ROWS))
#define SGC_MAX_HALO 4
#define SGC_MAX_IN_W (SGC_TILE_W + 2 * SGC_MAX_HALO)
#define SGC_MAX_IN_H (SGC_TILE_H + 2 * SGC_MAX_HALO)

/* the u16 tile with its halo of 2 * step: element idx in [0, in_w * in_h) is pixel
 * (x0 - halo + idx % in_w, y0 - halo + idx / in_w); outside the frame 0 (never read by the rule) */
SGC_HD uint16_t sgc_tile_load(int idx, const uint16_t *plane, int W, int H, int x0, int y0, int halo) {
	const int in_w = SGC_TILE_W + 2 * halo;
	const int ly = idx / in_w, lx = idx - ly * in_w;
	const int gx = x0 - halo + lx, gy = y0 - halo + ly;
	if (gx < 0 || gx >= W || gy < 0 || gy >= H)
		return 0;
	return plane[(int64_t)gy * W + gx];
}

struct SgcTileGet {
	const uint16_t *s;	/* in_w * in_h */
	int x0, y0, halo, in_w;
	SGC_HD_MEMBER uint32_t at(int xx, int yy) const {
		return s[(yy - y0 + halo) * in_w + (xx - x0 + halo)];
	}
};

/* ------------------------------------------------------------------ the rounds */

/*
 * The frame keeps its original values until the very end; the value the serial scan would have
 * left at a pixel lies in `state` while one of the pixel's two kind bits is set.  A pixel at scan
 * position p reads the corrected value of the neighbours before p and the original of the others,
 * which is what autoDetect's in-place loop sees.
 */
struct SgcStateGet {
	const uint16_t *plane;		/* the layer, W * H, original */
	const uint16_t *state;		/* the layer's corrected values */
	const uint32_t *hot, *cold;	/* kind bits, indexed by base + pixel */
	uint64_t base;			/* the layer's first bit */
	int64_t p;			/* the scan position of the pixel being decided */
	int W;
	SGC_HD_MEMBER uint32_t at(int xx, int yy) const {
		const int64_t q = (int64_t)yy * W + xx;
		if (q < p) {
			const uint64_t b = base + (uint64_t)q;
			const uint32_t w = SGC_LOAD_BITS(&hot[b >> 5]) | SGC_LOAD_BITS(&cold[b >> 5]);
			if ((w >> (b & 31)) & 1u)
				return state[q];
		}
		return plane[q];
	}
};

/* the pixels after (x, y) in scan order that have it in their 5x5 window: k in [0, 12) */
SGC_HD bool sgc_later(int k, int x, int y, int W, int H, int step, int *xx, int *yy) {
	const int i = 13 + k;	/* positions 13 .. 24 of the 5 x 5 window */
	*xx = x + (i % 5 - 2) * step;
	*yy = y + (i / 5 - 2) * step;
	return *yy >= 0 && *yy < H && *xx >= 0 && *xx < W;
}
