/*
 * sg_starmatch.h - new_star_match for one frame (include/sirilgpu.h, sg_starmatch), host + device:
 * the triangle match of atFindTrans with match.c's second try, atApplyTrans + atMatchLists, atCalcRMS,
 * atRecalcTrans and cvCalculH (findHomography with RANSAC, runKernel, refine), restated from
 * src/registration/matching/match.c:125-389, atpmatch.c and src/opencv/findHomography/{fundam,
 * modelest,calibration}.cpp.  tests/starmatch_ref.py is the literal numpy form and states the
 * contracts (tie rules, the reads past the winners, the eigen-solver); the constants carry the
 * reference's names.
 *
 * One frame is a chain of stages over a workspace of plain arrays (SgmWork: LDS in k_starmatch, heap
 * in a host program).  Every stage is called by all `nlanes` lanes with their `lane`; lane l works on
 * items l, l + nlanes, ..; SGM_SYNC() separates the stages (a workgroup barrier on the device, nothing
 * on the host, where nlanes = 1).  The serial parts (the 3 x 3 solves, percentiles, drops, the
 * generator, getSubset, the 4-point kernels, the Jacobi solves and the LM bookkeeping) run on lane 0;
 * every decision is published through the workspace, so all lanes branch alike.
 *
 * Sums over pairs run in one fixed order whatever nlanes is (sgm_sums): item i belongs to virtual
 * lane i % SGM_LANES, a virtual lane adds its items in ascending order from +0.0, and the SGM_LANES
 * partial sums fold by halving.  With -ffp-contract=off the host program and the kernel therefore give
 * the same bits; log (cvRANSACUpdateNumIters) is the one libm call whose last bit could differ, and
 * only cvRound of a quotient sees it.
 *
 * OpenCV's generator is its published multiply-with-carry (core/types_c.h: CV_RNG_COEFF 4164903690,
 * cvRandInt: state = (uint32)state * coeff + (state >> 32), output the low 32 bits), seeded with all
 * ones by CvModelEstimator2's constructor for every call.
 */
#pragma once
#include <float.h>
#include <math.h>
#include <stddef.h>
#include <stdint.h>
#include "../../include/sirilgpu.h"

#if defined(__HIPCC__)
#define SGM_HD __host__ __device__ static inline
#define SGM_HDM __host__ __device__ inline
#else
#define SGM_HD static inline
#define SGM_HDM inline
#endif
#if defined(__HIP_DEVICE_COMPILE__)
#define SGM_SYNC() __syncthreads()
#define SGM_INC(p) atomicAdd((p), 1)
#define SGM_ADD(p, v) atomicAdd((p), (v))
#else
#define SGM_SYNC() ((void)0)
#define SGM_INC(p) (++*(p))
#define SGM_ADD(p, v) (*(p) += (v))
#endif

#define SGM_LANES 256			/* virtual lanes of a sum = threads of a workgroup */
#define SGM_GROUP 8			/* sums folded together */
#define MAX_STARS_FITTED 2000
#define AT_MATCH_MINPAIRS 10
#define AT_MATCH_NBRIGHT 20
#define AT_TRIANGLE_RADIUS 0.002
#define AT_MATCH_RADIUS 5.0
#define AT_MATCH_MAXDIST 50.0
#define AT_MATCH_RATIO 0.8
#define AT_MATCH_REQUIRE_LINEAR 3
#define AT_MATCH_STARTN_LINEAR 6
#define AT_MATCH_PERCENTILE 0.70
#define AT_MATCH_NSIGMA 3.0
#define AT_MATCH_MAXITER 3
#define AT_MATCH_HALTSIGMA 1.0e-12
#define AT_MATCH_MINVOTES 2
#define ONE_STDEV_PERCENTILE 0.683
#define MATRIX_TOL 1.0e-12
#define SGM_MIN_SCALE 0.9
#define SGM_MAX_SCALE 1.1
#define SGM_RANSAC_THRESHOLD 3.0	/* defaultRANSACReprojThreshold */
#define SGM_RANSAC_CONFIDENCE 0.995
#define SGM_RANSAC_MAX_ITERS 2000
#define SGM_RANSAC_ATTEMPTS 300
#define SGM_LM_MAX_ITERS 10
#define SGM_JACOBI_SWEEPS 50
#define SGM_NTRI (AT_MATCH_NBRIGHT * (AT_MATCH_NBRIGHT - 1) * (AT_MATCH_NBRIGHT - 2) / 6)	/* 1140 */
#define SGM_CV_RNG_COEFF 4164903690u

/* integer scalars of the workspace */
enum { SGM_I_NTA = 0, SGM_I_NTB, SGM_I_NW, SGM_I_NP, SGM_I_STATE, SGM_I_NR, SGM_I_GOOD, SGM_I_SEL, SGM_I_BEST, SGM_I_ITER,
       SGM_I_NITERS, SGM_I_MODEL, SGM_I_NINL, SGM_I_LM, SGM_I_LG, SGM_I_FLAG, SGM_I_COUNT = 16 };
/* double scalars: the TRANS, sigma, the sums of one evaluation, RANSAC's models, refine's state */
enum { SGM_D_TR = 0, SGM_D_SIG = 6, SGM_D_SUM = 8, SGM_D_HCUR = 56, SGM_D_HBEST = 65, SGM_D_PARAM = 74, SGM_D_PREV = 82,
       SGM_D_JTJ = 90, SGM_D_JTE = 154, SGM_D_ERR = 162, SGM_D_PERR = 163, SGM_D_COUNT = 168 };
enum { SGM_ST_REFIT = 0, SGM_ST_DONE = 1, SGM_ST_FAIL = 2 };

/*
 * The workspace of one frame for lists of at most nmax stars, in this order (sgm_work_bytes):
 *   ax ay bx by   double [nmax] each   both lists' positions
 *   pa pb         int32 [nmax] each    the pairs under work: winners, then the matched lists
 *   U             72960 bytes, used twice:
 *                 - until the votes are cast: both triangle arrays, ba ca a_length as double
 *                   [2][1140], the three vertex indices packed in a uint32 [2][1140], and the order
 *                   by ba int32 [2][1140];
 *                 - afterwards (the triangles are dead once both vote matrices stand): dist double
 *                   [nmax], srt double [nmax], choice int32 [nmax], part double [8][256];
 *   dsc           double [168]         the scalars above
 *   vote          int32 [2][400]       with and without the scale test
 *   win br        int32 [5][20]        winners' votes / A / B, the bright stars' ids of A and B
 *   isc           int32 [16]
 *   mask tmask    uint8 [nmax] each    RANSAC's masks
 * At nmax = 2000 that is 161 968 bytes of the 163 840 a gfx950 workgroup has.
 */
struct SgmWork {
	double *ax, *ay, *bx, *by;
	int32_t *pa, *pb;
	double *tba, *tca, *tal;
	uint32_t *tidx;
	int32_t *tord;
	double *dist, *srt, *part;
	int32_t *choice;
	int32_t *vote, *win_v, *win_a, *win_b, *br_a, *br_b, *isc;
	double *dsc;
	unsigned char *mask, *tmask;
};

SGM_HD size_t sgm_up8(size_t v) {
	return (v + 7) & ~(size_t)7;
}
#define SGM_U_BYTES ((size_t)2 * SGM_NTRI * (3 * sizeof(double) + sizeof(uint32_t) + sizeof(int32_t)))

SGM_HD size_t sgm_u2_bytes(int nmax) {	/* U's second use */
	return (size_t)nmax * (2 * sizeof(double) + sizeof(int32_t)) + (size_t)SGM_GROUP * SGM_LANES * sizeof(double) + 8;
}

SGM_HD size_t sgm_work_bytes(int nmax) {
	const size_t u = SGM_U_BYTES > sgm_u2_bytes(nmax) ? SGM_U_BYTES : sgm_u2_bytes(nmax);
	return (size_t)nmax * 4 * sizeof(double) + sgm_up8((size_t)nmax * 2 * sizeof(int32_t)) + u +
			(size_t)(2 * 400 + 5 * AT_MATCH_NBRIGHT + SGM_I_COUNT) * sizeof(int32_t) + (size_t)SGM_D_COUNT * sizeof(double) +
			sgm_up8((size_t)nmax * 2);
}

SGM_HD SgmWork sgm_work(unsigned char *base, int nmax) {
	SgmWork w;
	const size_t n = (size_t)nmax;
	w.ax = (double *)base;
	w.ay = w.ax + n;
	w.bx = w.ay + n;
	w.by = w.bx + n;
	w.pa = (int32_t *)(w.by + n);
	w.pb = w.pa + n;
	unsigned char *u = (unsigned char *)w.pa + sgm_up8(n * 2 * sizeof(int32_t));
	w.tba = (double *)u;
	w.tca = w.tba + 2 * SGM_NTRI;
	w.tal = w.tca + 2 * SGM_NTRI;
	w.tidx = (uint32_t *)(w.tal + 2 * SGM_NTRI);
	w.tord = (int32_t *)(w.tidx + 2 * SGM_NTRI);
	w.dist = (double *)u;
	w.srt = w.dist + n;
	w.part = w.srt + n;
	w.choice = (int32_t *)(w.part + SGM_GROUP * SGM_LANES);
	const size_t ub = SGM_U_BYTES > sgm_u2_bytes(nmax) ? SGM_U_BYTES : sgm_u2_bytes(nmax);
	w.dsc = (double *)(u + ub);
	w.vote = (int32_t *)(w.dsc + SGM_D_COUNT);
	w.win_v = w.vote + 2 * 400;
	w.win_a = w.win_v + AT_MATCH_NBRIGHT;
	w.win_b = w.win_a + AT_MATCH_NBRIGHT;
	w.br_a = w.win_b + AT_MATCH_NBRIGHT;
	w.br_b = w.br_a + AT_MATCH_NBRIGHT;
	w.isc = w.br_b + AT_MATCH_NBRIGHT;
	w.mask = (unsigned char *)(w.isc + SGM_I_COUNT);
	w.tmask = w.mask + n;
	return w;
}

/* ---------------------------------------------------------------------------------- sums */

/* out[k] (workspace doubles) = the sum over items i < n of f(i)'s k-th term, K terms, in the fixed
 * order of this file's header.  Called by all lanes; ends synchronised. */
template <int K, class F>
SGM_HD void sgm_sums(const SgmWork &w, int lane, int nlanes, int n, const F &f, double *out) {
	for (int k0 = 0; k0 < K; k0 += SGM_GROUP) {
		const int kn = K - k0 < SGM_GROUP ? K - k0 : SGM_GROUP;
		for (int v = lane; v < SGM_LANES; v += nlanes) {
			double acc[SGM_GROUP];
			for (int k = 0; k < SGM_GROUP; k++)
				acc[k] = 0.;
			for (int i = v; i < n; i += SGM_LANES) {
				double t[K];
				f(i, t);
				for (int k = 0; k < kn; k++)
					acc[k] += t[k0 + k];
			}
			for (int k = 0; k < kn; k++)
				w.part[k * SGM_LANES + v] = acc[k];
		}
		SGM_SYNC();
		for (int s = SGM_LANES / 2; s >= 1; s >>= 1) {
			for (int v = lane; v < s; v += nlanes)
				for (int k = 0; k < kn; k++)
					w.part[k * SGM_LANES + v] += w.part[k * SGM_LANES + v + s];
			SGM_SYNC();
		}
		if (lane == 0)
			for (int k = 0; k < kn; k++)
				out[k0 + k] = w.part[k * SGM_LANES];
		SGM_SYNC();
	}
}

/* ---------------------------------------------------------------------------------- triangles */

/* the `rank` smallest of n keys by (key, index): dst[rank] = index for rank < keep */
SGM_HD void sgm_rank_select(const double *key, int n, int keep, int32_t *dst, int lane, int nlanes) {
	for (int i = lane; i < n; i += nlanes) {
		const double k = key[i];
		int r = 0;
		for (int j = 0; j < n && r < keep; j++)
			r += key[j] < k || (key[j] == k && j < i);
		if (r < keep)
			dst[r] = i;
	}
}

/* set_triangle for the t-th triangle in fill_triangle_array's order over nb stars given by ids */
SGM_HD void sgm_set_triangle(const double *x, const double *y, const int32_t *ids, int nb, int t, double *ba, double *ca,
		double *al, uint32_t *idx) {
	int s1 = 0, rest = t;
	for (;; s1++) {
		const int c = (nb - 1 - s1) * (nb - 2 - s1) / 2;
		if (rest < c)
			break;
		rest -= c;
	}
	int s2 = s1 + 1;
	for (;; s2++) {
		const int c = nb - 1 - s2;
		if (rest < c)
			break;
		rest -= c;
	}
	const int s3 = s2 + 1 + rest;
	const double x1 = x[ids[s1]], y1 = y[ids[s1]], x2 = x[ids[s2]], y2 = y[ids[s2]], x3 = x[ids[s3]], y3 = y[ids[s3]];
	const double d12 = sqrt((x1 - x2) * (x1 - x2) + (y1 - y2) * (y1 - y2));
	const double d23 = sqrt((x2 - x3) * (x2 - x3) + (y2 - y3) * (y2 - y3));
	const double d13 = sqrt((x1 - x3) * (x1 - x3) + (y1 - y3) * (y1 - y3));
	int ai, bi, ci;
	double a, b, c;
	if (d12 >= d23 && d12 >= d13) {
		ai = s3;
		a = d12;
		if (d23 >= d13) {
			bi = s1, b = d23, ci = s2, c = d13;
		} else {
			bi = s2, b = d13, ci = s1, c = d23;
		}
	} else if (d23 > d12 && d23 >= d13) {
		ai = s1;
		a = d23;
		if (d12 > d13) {
			bi = s3, b = d12, ci = s2, c = d13;
		} else {
			bi = s2, b = d13, ci = s3, c = d12;
		}
	} else {
		ai = s2;
		a = d13;
		if (d12 > d23) {
			bi = s3, b = d12, ci = s1, c = d23;
		} else {
			bi = s1, b = d23, ci = s3, c = d12;
		}
	}
	*al = a;
	*ba = a > 0.0 ? b / a : 1.0;
	*ca = a > 0.0 ? c / a : 1.0;
	*idx = (uint32_t)ai | ((uint32_t)bi << 8) | ((uint32_t)ci << 16);
}

/* find_ba_triangle over the A triangles in ba order */
SGM_HD int sgm_find_ba(const double *ba, const int32_t *ord, int num, double ba0) {
	int top = 0, bottom = num - 1 < 0 ? 0 : num - 1;
	while (bottom - top > 2) {
		const int mid = (top + bottom) / 2;
		if (ba[ord[mid]] < ba0)
			top = mid;
		else
			bottom = mid;
	}
	return ba[ord[top]] < ba0 ? bottom : top;
}

/* stars_to_triangles + prune for both lists, then make_vote_matrix once for both tries: vote[0] with
 * the scale test, vote[400] without.  n >= 6 stars in each list.  Ends synchronised. */
SGM_HD void sgm_triangles_votes(const SgmWork &w, int lane, int nlanes, const double *A, const double *B, int n, int nb) {
	/* the mags, staged where the distances will live */
	for (int i = lane; i < n; i += nlanes) {
		w.dist[i] = A[3 * (size_t)i + 2];
		w.srt[i] = B[3 * (size_t)i + 2];
	}
	SGM_SYNC();
	sgm_rank_select(w.dist, n, nb, w.br_a, lane, nlanes);
	sgm_rank_select(w.srt, n, nb, w.br_b, lane, nlanes);
	SGM_SYNC();
	const int nt = nb * (nb - 1) * (nb - 2) / 6;
	for (int t = lane; t < 2 * nt; t += nlanes) {
		const int L = t >= nt, u = L ? t - nt : t, o = L * SGM_NTRI + u;
		sgm_set_triangle(L ? w.bx : w.ax, L ? w.by : w.ay, L ? w.br_b : w.br_a, nb, u, &w.tba[o], &w.tca[o], &w.tal[o], &w.tidx[o]);
	}
	for (int c = lane; c < 2 * 400; c += nlanes)
		w.vote[c] = 0;
	SGM_SYNC();
	sgm_rank_select(w.tba, nt, nt, w.tord, lane, nlanes);
	sgm_rank_select(w.tba + SGM_NTRI, nt, nt, w.tord + SGM_NTRI, lane, nlanes);
	SGM_SYNC();
	if (lane == 0) {
		for (int L = 0; L < 2; L++) {
			int i = nt - 1;
			for (; i >= 0; i--)
				if (w.tba[L * SGM_NTRI + w.tord[L * SGM_NTRI + i]] <= AT_MATCH_RATIO)
					break;
			w.isc[SGM_I_NTA + L] = i < 0 ? 0 : i;	/* numtriangles = i, as written */
		}
	}
	SGM_SYNC();
	const int nta = w.isc[SGM_I_NTA], ntb = w.isc[SGM_I_NTB];
	const double rad2 = AT_TRIANGLE_RADIUS * AT_TRIANGLE_RADIUS;
	for (int j = lane; j < ntb && nta > 0; j += nlanes) {
		const int tb = SGM_NTRI + w.tord[SGM_NTRI + j];
		const double ba_B = w.tba[tb], ca_B = w.tca[tb];
		const double ba_min = ba_B - AT_TRIANGLE_RADIUS, ba_max = ba_B + AT_TRIANGLE_RADIUS;
		const uint32_t ib = w.tidx[tb];
		for (int i = sgm_find_ba(w.tba, w.tord, nta, ba_min); i < nta; i++) {
			const int ta = w.tord[i];
			const double ba_A = w.tba[ta], ca_A = w.tca[ta];
			if (ba_A > ba_max)
				break;
			if ((ba_A - ba_B) * (ba_A - ba_B) + (ca_A - ca_B) * (ca_A - ca_B) < rad2) {
				const uint32_t ia = w.tidx[ta];
				const double ratio = w.tal[ta] / w.tal[tb];
				const int scaled = !(ratio < SGM_MIN_SCALE || ratio > SGM_MAX_SCALE);
				for (int s = 0; s < 24; s += 8) {
					const int cell = (int)((ia >> s) & 255u) * nb + (int)((ib >> s) & 255u);
					SGM_INC(&w.vote[400 + cell]);
					if (scaled)
						SGM_INC(&w.vote[cell]);
				}
			}
		}
	}
	SGM_SYNC();
}

/* top_vote_getters in closed form over one vote matrix, the cut at AT_MATCH_MINVOTES, and the winners
 * as pairs of star ids in pa / pb; isc[SGM_I_NW] = their number.  Ends synchronised. */
SGM_HD void sgm_winners(const SgmWork &w, int lane, int nlanes, const int32_t *vote, int nb) {
	for (int k = lane; k < nb; k += nlanes) {
		w.win_v[k] = 0;
		w.win_a[k] = w.win_b[k] = -1;
	}
	SGM_SYNC();
	for (int c = lane; c < nb * nb; c += nlanes) {
		const int v = vote[c];
		if (v <= 0)
			continue;
		int r = 0;
		for (int d = 0; d < nb * nb && r < nb; d++)
			r += vote[d] > v || (vote[d] == v && d < c);
		if (r < nb) {
			w.win_v[r] = v;
			w.win_a[r] = c / nb;
			w.win_b[r] = c % nb;
		}
	}
	SGM_SYNC();
	if (lane == 0) {
		int nw = nb;
		for (int i = 0; i < nb; i++)
			if (w.win_v[i] < AT_MATCH_MINVOTES) {
				nw = i;
				break;
			}
		for (int i = 0; i < nw; i++) {
			w.pa[i] = w.br_a[w.win_a[i]];
			w.pb[i] = w.br_b[w.win_b[i]];
		}
		w.isc[SGM_I_NW] = nw;
	}
	SGM_SYNC();
}

/* ---------------------------------------------------------------------------------- TRANS */

/* gauss_matrix with gauss_pivot, num = 3, on copies */
SGM_HD int sgm_gauss3(const double m0[3][3], const double v0[3], double sol[3]) {
	double m[3][3], v[3], big[3];
	for (int i = 0; i < 3; i++) {
		v[i] = v0[i];
		for (int j = 0; j < 3; j++)
			m[i][j] = m0[i][j];
	}
	for (int i = 0; i < 3; i++) {
		big[i] = fabs(m[i][0]);
		for (int j = 1; j < 3; j++)
			if (fabs(m[i][j]) > big[i])
				big[i] = fabs(m[i][j]);
		if (big[i] == 0.0)
			return 0;
	}
	for (int i = 0; i < 2; i++) {
		int pr = i;
		double bg = fabs(m[i][i] / big[i]);
		for (int r = i + 1; r < 3; r++) {
			const double o = fabs(m[r][i] / big[r]);
			if (o > bg) {
				bg = o;
				pr = r;
			}
		}
		if (pr != i) {
			for (int c = i; c < 3; c++) {
				const double t = m[pr][c];
				m[pr][c] = m[i][c];
				m[i][c] = t;
			}
			double t = v[pr];
			v[pr] = v[i];
			v[i] = t;
			t = big[pr];
			big[pr] = big[i];
			big[i] = t;
		}
		if (fabs(m[i][i] / big[i]) < MATRIX_TOL)
			return 0;
		for (int j = i + 1; j < 3; j++) {
			const double f = m[j][i] / m[i][i];
			for (int k = i + 1; k < 3; k++)
				m[j][k] -= f * m[i][k];
			v[j] -= f * v[i];
		}
	}
	if (fabs(m[2][2] / big[2]) < MATRIX_TOL)
		return 0;
	sol[2] = v[2] / m[2][2];
	for (int i = 1; i >= 0; i--) {
		double s = 0.0;
		for (int j = i + 1; j < 3; j++)
			s += m[i][j] * sol[j];
		sol[i] = (v[i] - s) / m[i][i];
	}
	return 1;
}

/* the sums of calc_trans_linear for pair i */
struct SgmTransTerms {
	const double *ax, *ay, *bx, *by;
	const int32_t *pa, *pb;
	SGM_HDM void operator()(int i, double *t) const {
		const double x1 = ax[pa[i]], y1 = ay[pa[i]], x2 = bx[pb[i]], y2 = by[pb[i]];
		t[0] = 1.0;
		t[1] = x1;
		t[2] = x2;
		t[3] = y1;
		t[4] = y2;
		t[5] = x1 * x1;
		t[6] = y1 * y1;
		t[7] = x1 * x2;
		t[8] = x1 * y1;
		t[9] = x1 * y2;
		t[10] = y1 * x2;
		t[11] = y1 * y2;
	}
};

/* calc_trans_linear over the first npairs pairs -> dsc[SGM_D_TR ..]; 0 = singular.  Ends synchronised. */
SGM_HD int sgm_calc_trans(const SgmWork &w, int lane, int nlanes, int npairs) {
	const SgmTransTerms f = {w.ax, w.ay, w.bx, w.by, w.pa, w.pb};
	sgm_sums<12>(w, lane, nlanes, npairs, f, w.dsc + SGM_D_SUM);
	if (lane == 0) {
		const double *s = w.dsc + SGM_D_SUM;
		const double m[3][3] = {{s[5], s[8], s[1]}, {s[8], s[6], s[3]}, {s[1], s[3], s[0]}};
		const double vx[3] = {s[7], s[10], s[2]}, vy[3] = {s[9], s[11], s[4]};
		double abc[3], def[3];
		const int ok = sgm_gauss3(m, vx, abc) && sgm_gauss3(m, vy, def);
		if (ok) {
			double *tr = w.dsc + SGM_D_TR;
			tr[0] = abc[2];
			tr[1] = abc[0];
			tr[2] = abc[1];
			tr[3] = def[2];
			tr[4] = def[0];
			tr[5] = def[1];
		}
		w.isc[SGM_I_MODEL] = ok;
	}
	SGM_SYNC();
	const int ok = w.isc[SGM_I_MODEL];
	SGM_SYNC();
	return ok;
}

SGM_HD double sgm_percentile(const double *srt, int num, double perc) {
	int index = (int)floor(num * perc + 0.5);
	if (index >= num)
		index = num - 1;
	return srt[index];
}

/* order-preserving drop of the pairs whose dist exceeds lim (lane 0): the new count */
SGM_HD int sgm_drop(const SgmWork &w, int nr, double lim) {
	int k = 0;
	for (int i = 0; i < nr; i++)
		if (!(w.dist[i] > lim)) {
			w.pa[k] = w.pa[i];
			w.pb[k] = w.pb[i];
			w.dist[k] = w.dist[i];
			k++;
		}
	return k;
}

/* iter_trans over the pairs pa / pb [nbright]: 1 = a TRANS in dsc[SGM_D_TR ..], its nr in
 * isc[SGM_I_NR] (the pairs left are the first nr) and sig in dsc[SGM_D_SIG].  Ends synchronised. */
SGM_HD int sgm_iter_trans(const SgmWork &w, int lane, int nlanes, int nbright, int recalc) {
	if (nbright < AT_MATCH_REQUIRE_LINEAR)
		return 0;
	const int initial = recalc ? nbright : AT_MATCH_STARTN_LINEAR;
	if (initial > nbright)
		return 0;	/* the reference reads past the winners here */
	if (!sgm_calc_trans(w, lane, nlanes, initial))
		return 0;
	int nr = nbright, ok = 1;
	for (int it = 0; it < AT_MATCH_MAXITER;) {
		const double *tr = w.dsc + SGM_D_TR;
		for (int i = lane; i < nr; i += nlanes) {
			const double x = w.ax[w.pa[i]], y = w.ay[w.pa[i]];
			const double xd = (tr[0] + tr[1] * x + tr[2] * y) - w.bx[w.pb[i]], yd = (tr[3] + tr[4] * x + tr[5] * y) - w.by[w.pb[i]];
			w.dist[i] = xd * xd + yd * yd;
		}
		SGM_SYNC();
		for (int i = lane; i < nr; i += nlanes) {
			const double d = w.dist[i];
			int r = 0;
			for (int j = 0; j < nr; j++)
				r += w.dist[j] < d || (w.dist[j] == d && j < i);
			w.srt[r] = d;
		}
		SGM_SYNC();
		if (lane == 0) {
			int n1 = sgm_drop(w, nr, AT_MATCH_MAXDIST * AT_MATCH_MAXDIST), nb = nr - n1, st = SGM_ST_REFIT;
			double sigma = 0.0;
			if (n1 >= 2)
				sigma = sgm_percentile(w.srt, n1, AT_MATCH_PERCENTILE);
			if (n1 == 0) {
				st = SGM_ST_FAIL;
			} else if (sigma <= AT_MATCH_HALTSIGMA) {
				st = SGM_ST_DONE;
			} else {
				const int n2 = sgm_drop(w, n1, AT_MATCH_NSIGMA * sigma);
				nb += n1 - n2;
				n1 = n2;
				if (nb == 0)
					st = SGM_ST_DONE;
				else if (n1 < AT_MATCH_REQUIRE_LINEAR)
					st = SGM_ST_FAIL;
			}
			w.isc[SGM_I_NR] = n1;
			w.isc[SGM_I_STATE] = st;
		}
		SGM_SYNC();
		nr = w.isc[SGM_I_NR];
		const int st = w.isc[SGM_I_STATE];
		SGM_SYNC();
		if (st == SGM_ST_FAIL && nr == 0)
			return 0;
		if (st != SGM_ST_REFIT) {
			ok = st == SGM_ST_DONE;
			break;
		}
		if (!sgm_calc_trans(w, lane, nlanes, nr))
			return 0;
		it++;
	}
	if (lane == 0) {
		w.dsc[SGM_D_SIG] = sgm_percentile(w.srt, nr, ONE_STDEV_PERCENTILE);
		w.isc[SGM_I_NR] = nr;
	}
	SGM_SYNC();
	return ok;
}

/* ---------------------------------------------------------------------------------- match lists */

/* the matched pairs held in choice (A star -> its B star or -1, one A per B) into pa / pb in ascending
 * B id; isc[SGM_I_NP] = their number.  Ends synchronised. */
SGM_HD void sgm_pairs_from_choice(const SgmWork &w, int lane, int nlanes, int n) {
	if (lane == 0)
		w.isc[SGM_I_NP] = 0;
	SGM_SYNC();
	int cnt = 0;
	for (int a = lane; a < n; a += nlanes) {
		const int b = w.choice[a];
		if (b < 0)
			continue;
		int r = 0;
		for (int a2 = 0; a2 < n; a2++)
			r += w.choice[a2] >= 0 && w.choice[a2] < b;
		w.pa[r] = a;
		w.pb[r] = b;
		cnt++;
	}
	if (cnt)
		SGM_ADD(&w.isc[SGM_I_NP], cnt);
	SGM_SYNC();
}

/* atApplyTrans on all of A and atMatchLists in closed form; the pairs go to pa / pb in ascending B id,
 * isc[SGM_I_NP] = their number.  Ends synchronised. */
SGM_HD void sgm_match_lists(const SgmWork &w, int lane, int nlanes, int n) {
	const double *tr = w.dsc + SGM_D_TR;
	const double radius = AT_MATCH_RADIUS, limit = radius * radius;
	int32_t *keep = (int32_t *)w.srt;	/* per B star the A star that keeps it */
	for (int a = lane; a < n; a += nlanes) {
		const double x = w.ax[a], y = w.ay[a];
		const double Ax = tr[0] + tr[1] * x + tr[2] * y, Ay = tr[3] + tr[4] * x + tr[5] * y;
		const double Axm = Ax - radius, Axp = Ax + radius, Aym = Ay - radius, Ayp = Ay + radius;
		int best = -1;
		double bd = 0.0;
		for (int b = 0; b < n; b++) {
			const double Bx = w.bx[b], By = w.by[b];
			if (Bx < Axm || Bx > Axp || By < Aym || By > Ayp)
				continue;
			const double dx = Ax - Bx, dy = Ay - By, d = dx * dx + dy * dy;
			if (!(d < limit))
				continue;
			if (best < 0 || d < bd || (d == bd && Bx < w.bx[best])) {	/* equal x: the smaller id stays */
				best = b;
				bd = d;
			}
		}
		w.choice[a] = best;
		w.dist[a] = bd;
	}
	SGM_SYNC();
	for (int b = lane; b < n; b += nlanes) {
		int best = -1;
		double bd = 0.0;
		for (int a = 0; a < n; a++)
			if (w.choice[a] == b && (best < 0 || w.dist[a] < bd)) {
				best = a;
				bd = w.dist[a];
			}
		keep[b] = best;
	}
	SGM_SYNC();
	/* an A star whose B star went to another is unmatched; choice now holds the matched pairs */
	for (int a = lane; a < n; a += nlanes)
		if (w.choice[a] >= 0 && keep[w.choice[a]] != a)
			w.choice[a] = -1;
	SGM_SYNC();
	sgm_pairs_from_choice(w, lane, nlanes, n);
}

/* atCalcRMS's two passes over the matched pairs: (dx^2, dy^2, tossed) with the clip of the second */
struct SgmRmsTerms {
	const SgmWork *w;
	int clip;
	double xlim, ylim;
	SGM_HDM void operator()(int i, double *t) const {
		const double *tr = w->dsc + SGM_D_TR;
		const double x = w->ax[w->pa[i]], y = w->ay[w->pa[i]];
		const double dx = w->bx[w->pb[i]] - (tr[0] + tr[1] * x + tr[2] * y), dy = w->by[w->pb[i]] - (tr[3] + tr[4] * x + tr[5] * y);
		const double dx2 = dx * dx, dy2 = dy * dy;
		const int in = !clip || (dx2 < xlim && dy2 < ylim);
		t[0] = in ? dx2 : 0.0;
		t[1] = in ? dy2 : 0.0;
		t[2] = in ? 0.0 : 1.0;
	}
};

/* ---------------------------------------------------------------------------------- the eigen-solver */

/* cyclic Jacobi on a symmetric N x N matrix: a's diagonal becomes the eigenvalues, column k of v the
 * k-th vector (tests/starmatch_ref.py, jacobi, is the same loop) */
template <int N>
SGM_HD void sgm_jacobi(double a[N][N], double v[N][N]) {
	for (int i = 0; i < N; i++)
		for (int j = 0; j < N; j++)
			v[i][j] = i == j ? 1.0 : 0.0;
	for (int sweep = 0; sweep < SGM_JACOBI_SWEEPS; sweep++) {
		double off = 0.0;
		for (int p = 0; p < N - 1; p++)
			for (int q = p + 1; q < N; q++)
				off += fabs(a[p][q]);
		if (off == 0.0)
			break;
		for (int p = 0; p < N - 1; p++)
			for (int q = p + 1; q < N; q++) {
				const double apq = a[p][q];
				if (apq == 0.0)
					continue;
				const double g = 100.0 * fabs(apq);
				if (fabs(a[p][p]) + g == fabs(a[p][p]) && fabs(a[q][q]) + g == fabs(a[q][q])) {
					a[p][q] = a[q][p] = 0.0;
					continue;
				}
				const double theta = (a[q][q] - a[p][p]) / (2.0 * apq);
				double t = 1.0 / (fabs(theta) + sqrt(theta * theta + 1.0));
				if (theta < 0.0)
					t = -t;
				const double c = 1.0 / sqrt(t * t + 1.0), s = t * c, tau = s / (1.0 + c);
				a[p][p] -= t * apq;
				a[q][q] += t * apq;
				a[p][q] = a[q][p] = 0.0;
				for (int r = 0; r < N; r++)
					if (r != p && r != q) {
						const double arp = a[r][p], arq = a[r][q];
						a[r][p] = a[p][r] = arp - s * (arq + tau * arp);
						a[r][q] = a[q][r] = arq + s * (arp - tau * arq);
					}
				for (int r = 0; r < N; r++) {
					const double vrp = v[r][p], vrq = v[r][q];
					v[r][p] = vrp - s * (vrq + tau * vrp);
					v[r][q] = vrq + s * (vrp - tau * vrq);
				}
			}
	}
}

/* ---------------------------------------------------------------------------------- the homography */

/* the matched pairs as cvCalculH sees them: Point2f, widened; sel = the inliers' pair indices or NULL */
struct SgmPoints {
	const SgmWork *w;
	const int32_t *sel;
	SGM_HDM void get(int i, double *Mx, double *My, double *mx, double *my) const {
		const int p = sel ? sel[i] : i;
		*Mx = (double)(float)w->ax[w->pa[p]];
		*My = (double)(float)w->ay[w->pa[p]];
		*mx = (double)(float)w->bx[w->pb[p]];
		*my = (double)(float)w->by[w->pb[p]];
	}
};

SGM_HD int sgm_check_subset(const double *px, const double *py, int count) {
	for (int i = 0; i < count; i++)
		for (int j = 0; j < i; j++) {
			const double dx1 = px[j] - px[i], dy1 = py[j] - py[i];
			for (int k = 0; k < j; k++) {
				const double dx2 = px[k] - px[i], dy2 = py[k] - py[i];
				if (fabs(dx2 * dy1 - dy2 * dx1) <= FLT_EPSILON * (fabs(dx1) + fabs(dy1) + fabs(dx2) + fabs(dy2)))
					return 0;
			}
		}
	return 1;
}

SGM_HD uint32_t sgm_rand(uint64_t *state) {
	*state = (uint64_t)(uint32_t)*state * SGM_CV_RNG_COEFF + (*state >> 32);
	return (uint32_t)*state;
}

/* getSubset(.., 300), checkPartialSubsets off: 4 distinct pairs whose points pass checkSubset in both sets */
SGM_HD int sgm_get_subset(uint64_t *rng, const SgmPoints &pts, int count, double Mx[4], double My[4], double mx[4], double my[4]) {
	for (int iters = 0; iters < SGM_RANSAC_ATTEMPTS; iters++) {
		int idx[4];
		for (int i = 0; i < 4;) {
			const int k = (int)(sgm_rand(rng) % (uint32_t)count);
			int j = 0;
			for (; j < i; j++)
				if (idx[j] == k)
					break;
			if (j < i)
				continue;
			idx[i] = k;
			pts.get(k, &Mx[i], &My[i], &mx[i], &my[i]);
			i++;
		}
		if (sgm_check_subset(Mx, My, 4) && sgm_check_subset(mx, my, 4))
			return 1;
	}
	return 0;
}

/* runKernel's terms: the centroids, the absolute deviations, and LtL's upper triangle */
struct SgmCentroidTerms {
	SgmPoints pts;
	SGM_HDM void operator()(int i, double *t) const {
		pts.get(i, &t[2], &t[3], &t[0], &t[1]);	/* cm.x cm.y cM.x cM.y */
	}
};
struct SgmSpreadTerms {
	SgmPoints pts;
	const double *c;	/* cm.x cm.y cM.x cM.y */
	SGM_HDM void operator()(int i, double *t) const {
		double Mx, My, mx, my;
		pts.get(i, &Mx, &My, &mx, &my);
		t[0] = fabs(mx - c[0]);
		t[1] = fabs(my - c[1]);
		t[2] = fabs(Mx - c[2]);
		t[3] = fabs(My - c[3]);
	}
};
struct SgmLtLTerms {
	SgmPoints pts;
	const double *c, *s;	/* the centroids; the scales sm.x sm.y sM.x sM.y */
	SGM_HDM void operator()(int i, double *t) const {
		double Mx, My, mx, my;
		pts.get(i, &Mx, &My, &mx, &my);
		const double x = (mx - c[0]) * s[0], y = (my - c[1]) * s[1], X = (Mx - c[2]) * s[2], Y = (My - c[3]) * s[3];
		const double Lx[9] = {X, Y, 1, 0, 0, 0, -x * X, -x * Y, -x}, Ly[9] = {0, 0, 0, X, Y, 1, -y * X, -y * Y, -y};
		int n = 0;
		for (int j = 0; j < 9; j++)
			for (int k = j; k < 9; k++)
				t[n++] = Lx[j] * Lx[k] + Ly[j] * Ly[k];
	}
};

/* runKernel after its sums: the eigenvector of LtL's smallest eigenvalue, denormalised, over h22 */
SGM_HD void sgm_kernel_finish(const double *c, const double *s, const double *ltl45, double *H) {
	double a[9][9], v[9][9];
	int n = 0;
	for (int j = 0; j < 9; j++)
		for (int k = j; k < 9; k++)
			a[j][k] = a[k][j] = ltl45[n++];
	sgm_jacobi<9>(a, v);
	int small = 0;
	for (int k = 1; k < 9; k++)
		if (a[k][k] < a[small][small])
			small = k;
	double h0[9], tmp[9], h[9];
	for (int r = 0; r < 9; r++)
		h0[r] = v[r][small];
	const double inv[9] = {1. / s[0], 0, c[0], 0, 1. / s[1], c[1], 0, 0, 1};
	const double n2[9] = {s[2], 0, -c[2] * s[2], 0, s[3], -c[3] * s[3], 0, 0, 1};
	for (int i = 0; i < 3; i++)
		for (int j = 0; j < 3; j++)
			tmp[3 * i + j] = inv[3 * i] * h0[j] + inv[3 * i + 1] * h0[3 + j] + inv[3 * i + 2] * h0[6 + j];
	for (int i = 0; i < 3; i++)
		for (int j = 0; j < 3; j++)
			h[3 * i + j] = tmp[3 * i] * n2[j] + tmp[3 * i + 1] * n2[3 + j] + tmp[3 * i + 2] * n2[6 + j];
	const double sc = 1. / h[8];
	for (int r = 0; r < 9; r++)
		H[r] = h[r] * sc;
}

/* the deviations' test and the scales of runKernel, in place: 0 = degenerate */
SGM_HD int sgm_kernel_scales(double *s, int count) {
	for (int k = 0; k < 4; k++)
		if (fabs(s[k]) < DBL_EPSILON)
			return 0;
	for (int k = 0; k < 4; k++)
		s[k] = count / s[k];
	return 1;
}

/* runKernel on a 4-point sample, sums in order (one lane) */
SGM_HD int sgm_kernel4(const double Mx[4], const double My[4], const double mx[4], const double my[4], double *H) {
	double c[4] = {0, 0, 0, 0}, s[4] = {0, 0, 0, 0}, ltl[45];
	for (int i = 0; i < 4; i++) {
		c[0] += mx[i];
		c[1] += my[i];
		c[2] += Mx[i];
		c[3] += My[i];
	}
	for (int k = 0; k < 4; k++)
		c[k] /= 4;
	for (int i = 0; i < 4; i++) {
		s[0] += fabs(mx[i] - c[0]);
		s[1] += fabs(my[i] - c[1]);
		s[2] += fabs(Mx[i] - c[2]);
		s[3] += fabs(My[i] - c[3]);
	}
	if (!sgm_kernel_scales(s, 4))
		return 0;
	for (int n = 0; n < 45; n++)
		ltl[n] = 0.0;
	for (int i = 0; i < 4; i++) {
		const double x = (mx[i] - c[0]) * s[0], y = (my[i] - c[1]) * s[1], X = (Mx[i] - c[2]) * s[2], Y = (My[i] - c[3]) * s[3];
		const double Lx[9] = {X, Y, 1, 0, 0, 0, -x * X, -x * Y, -x}, Ly[9] = {0, 0, 0, X, Y, 1, -y * X, -y * Y, -y};
		int n = 0;
		for (int j = 0; j < 9; j++)
			for (int k = j; k < 9; k++)
				ltl[n++] += Lx[j] * Lx[k] + Ly[j] * Ly[k];
	}
	sgm_kernel_finish(c, s, ltl, H);
	return 1;
}

/* cvRANSACUpdateNumIters for 4 model points; pow(1 - ep, 4) as two squarings */
SGM_HD int sgm_update_num_iters(double p, double ep, int max_iters) {
	p = p < 0. ? 0. : p > 1. ? 1. : p;
	ep = ep < 0. ? 0. : ep > 1. ? 1. : ep;
	double num = 1. - p > DBL_MIN ? 1. - p : DBL_MIN;
	const double wv = 1. - ep;
	double denom = 1. - (wv * wv) * (wv * wv);
	if (denom < DBL_MIN)
		return 0;
	num = log(num);
	denom = log(denom);
	return denom >= 0 || -num >= max_iters * (-denom) ? max_iters : (int)rint(num / denom);
}

/* refine's terms at param h: JtJ's upper triangle (36), JtErr (8), errNorm; or errNorm alone */
struct SgmRefineTerms {
	SgmPoints pts;
	const double *h;
	int full;
	SGM_HDM void operator()(int i, double *t) const {
		double Mx, My, mx, my;
		pts.get(i, &Mx, &My, &mx, &my);
		double ww = h[6] * Mx + h[7] * My + 1.;
		ww = fabs(ww) > DBL_EPSILON ? 1. / ww : 0;
		const double xi = (h[0] * Mx + h[1] * My + h[2]) * ww, yi = (h[3] * Mx + h[4] * My + h[5]) * ww;
		const double e0 = xi - mx, e1 = yi - my;
		if (!full) {
			t[0] = e0 * e0 + e1 * e1;
			return;
		}
		const double J0[8] = {Mx * ww, My * ww, ww, 0, 0, 0, -Mx * ww * xi, -My * ww * xi};
		const double J1[8] = {0, 0, 0, Mx * ww, My * ww, ww, -Mx * ww * yi, -My * ww * yi};
		int n = 0;
		for (int j = 0; j < 8; j++)
			for (int k = j; k < 8; k++)
				t[n++] = J0[j] * J0[k] + J1[j] * J1[k];
		for (int j = 0; j < 8; j++)
			t[36 + j] = J0[j] * e0 + J1[j] * e1;
		t[44] = e0 * e0 + e1 * e1;
	}
};

/* CvLevMarq::step (lane 0): param = prev - pinv(JtJ with its diagonal times 1 + 10^lg) JtErr.  lambda
 * comes from a table of powers of ten, not from exp(lg * log(10)) */
SGM_HD void sgm_lm_step(const double *jtj64, const double *jte, const double *prev, int lg, double *param) {
	const double P10[34] = {1e-16, 1e-15, 1e-14, 1e-13, 1e-12, 1e-11, 1e-10, 1e-9, 1e-8, 1e-7, 1e-6, 1e-5, 1e-4, 1e-3, 1e-2, 1e-1, 1e0,
		1e1, 1e2, 1e3, 1e4, 1e5, 1e6, 1e7, 1e8, 1e9, 1e10, 1e11, 1e12, 1e13, 1e14, 1e15, 1e16, 1e17};
	const double lambda = P10[lg + 16];
	double a[8][8], v[8][8], delta[8];
	for (int i = 0; i < 8; i++)
		for (int j = 0; j < 8; j++)
			a[i][j] = jtj64[i * 8 + j];
	for (int i = 0; i < 8; i++)
		a[i][i] *= 1. + lambda;
	sgm_jacobi<8>(a, v);
	double thr = 0.0;
	for (int i = 0; i < 8; i++)
		thr += fabs(a[i][i]);
	thr *= 2 * DBL_EPSILON;
	for (int r = 0; r < 8; r++)
		delta[r] = 0.0;
	for (int k = 0; k < 8; k++)
		if (fabs(a[k][k]) > thr) {
			double dot = 0.0;
			for (int r = 0; r < 8; r++)
				dot += v[r][k] * jte[r];
			dot /= a[k][k];
			for (int r = 0; r < 8; r++)
				delta[r] += v[r][k] * dot;
		}
	for (int i = 0; i < 8; i++)
		param[i] = prev[i] - delta[i];
}

/* CvHomographyEstimator::refine on the count points of pts, from and to dsc[SGM_D_HBEST ..];
 * isc[SGM_I_LM] = the iterations.  Ends synchronised. */
SGM_HD void sgm_refine(const SgmWork &w, int lane, int nlanes, const SgmPoints &pts, int count) {
	double *d = w.dsc;
	if (lane == 0) {
		for (int i = 0; i < 8; i++)
			d[SGM_D_PARAM + i] = d[SGM_D_HBEST + i];
		w.isc[SGM_I_LG] = -3;
		w.isc[SGM_I_LM] = 0;
	}
	SGM_SYNC();
	SgmRefineTerms f = {pts, d + SGM_D_PARAM, 1};
	for (;;) {
		f.full = 1;
		sgm_sums<45>(w, lane, nlanes, count, f, d + SGM_D_SUM);
		if (lane == 0) {
			int n = 0;
			for (int j = 0; j < 8; j++)
				for (int k = j; k < 8; k++)
					d[SGM_D_JTJ + j * 8 + k] = d[SGM_D_JTJ + k * 8 + j] = d[SGM_D_SUM + n++];
			for (int j = 0; j < 8; j++)
				d[SGM_D_JTE + j] = d[SGM_D_SUM + 36 + j];
			if (w.isc[SGM_I_LM] == 0)
				d[SGM_D_ERR] = d[SGM_D_SUM + 44];	/* later rounds keep the errNorm of the accepted step */
			for (int i = 0; i < 8; i++)
				d[SGM_D_PREV + i] = d[SGM_D_PARAM + i];
			sgm_lm_step(d + SGM_D_JTJ, d + SGM_D_JTE, d + SGM_D_PREV, w.isc[SGM_I_LG], d + SGM_D_PARAM);
			d[SGM_D_PERR] = d[SGM_D_ERR];
		}
		SGM_SYNC();
		f.full = 0;
		for (;;) {
			sgm_sums<1>(w, lane, nlanes, count, f, d + SGM_D_SUM);
			if (lane == 0) {
				d[SGM_D_ERR] = d[SGM_D_SUM];
				int again = 0;
				if (d[SGM_D_ERR] > d[SGM_D_PERR] && ++w.isc[SGM_I_LG] <= 16) {
					sgm_lm_step(d + SGM_D_JTJ, d + SGM_D_JTE, d + SGM_D_PREV, w.isc[SGM_I_LG], d + SGM_D_PARAM);
					again = 1;
				}
				w.isc[SGM_I_FLAG] = again;
			}
			SGM_SYNC();
			const int again = w.isc[SGM_I_FLAG];
			SGM_SYNC();
			if (!again)
				break;
		}
		if (lane == 0) {
			const int lg = w.isc[SGM_I_LG] - 1;
			w.isc[SGM_I_LG] = lg > -16 ? lg : -16;
			int done = ++w.isc[SGM_I_LM] >= SGM_LM_MAX_ITERS;
			if (!done) {
				double num = 0.0, den = 0.0;
				for (int i = 0; i < 8; i++) {
					const double df = d[SGM_D_PARAM + i] - d[SGM_D_PREV + i];
					num += df * df;
					den += d[SGM_D_PREV + i] * d[SGM_D_PREV + i];
				}
				done = sqrt(num) / sqrt(den) < DBL_EPSILON;
			}
			w.isc[SGM_I_FLAG] = done;
		}
		SGM_SYNC();
		const int done = w.isc[SGM_I_FLAG];
		SGM_SYNC();
		if (done)
			break;
	}
	if (lane == 0)
		for (int i = 0; i < 8; i++)
			d[SGM_D_HBEST + i] = d[SGM_D_PARAM + i];
	SGM_SYNC();
}

/* cvCalculH over the count >= 5 matched pairs: 1 = H in dsc[SGM_D_HBEST ..], isc[SGM_I_BEST] inliers,
 * isc[SGM_I_ITER] RANSAC iterations, isc[SGM_I_LM] refine's.  Ends synchronised. */
SGM_HD int sgm_homography(const SgmWork &w, int lane, int nlanes, int count) {
	const SgmPoints all = {&w, nullptr};
	double *d = w.dsc;
	uint64_t rng = ~(uint64_t)0;	/* cvRNG(-1); lane 0's */
	if (lane == 0) {
		w.isc[SGM_I_ITER] = 0;
		w.isc[SGM_I_NITERS] = SGM_RANSAC_MAX_ITERS;
		w.isc[SGM_I_BEST] = 0;
		w.isc[SGM_I_SEL] = 0;
		w.isc[SGM_I_LM] = 0;
	}
	SGM_SYNC();
	for (;;) {
		const int iter = w.isc[SGM_I_ITER], niters = w.isc[SGM_I_NITERS];
		SGM_SYNC();
		if (iter >= niters)
			break;
		if (lane == 0) {
			double Mx[4], My[4], mx[4], my[4];
			int flag = 0, model = 0;
			if (!sgm_get_subset(&rng, all, count, Mx, My, mx, my))
				flag = iter == 0 ? 2 : 1;
			else
				model = sgm_kernel4(Mx, My, mx, my, d + SGM_D_HCUR);
			w.isc[SGM_I_FLAG] = flag;
			w.isc[SGM_I_MODEL] = model;
			w.isc[SGM_I_GOOD] = 0;
		}
		SGM_SYNC();
		const int flag = w.isc[SGM_I_FLAG], model = w.isc[SGM_I_MODEL];
		if (flag == 2)
			return 0;
		if (flag == 1)
			break;
		if (model) {
			const double *H = d + SGM_D_HCUR;
			unsigned char *tm = w.isc[SGM_I_SEL] ? w.mask : w.tmask;
			int good = 0;
			for (int i = lane; i < count; i += nlanes) {
				double Mx, My, mx, my;
				all.get(i, &Mx, &My, &mx, &my);
				const double ww = 1. / (H[6] * Mx + H[7] * My + 1.);
				const double dx = (H[0] * Mx + H[1] * My + H[2]) * ww - mx, dy = (H[3] * Mx + H[4] * My + H[5]) * ww - my;
				const int in = (float)(dx * dx + dy * dy) <= SGM_RANSAC_THRESHOLD * SGM_RANSAC_THRESHOLD;
				tm[i] = (unsigned char)in;
				good += in;
			}
			if (good)
				SGM_ADD(&w.isc[SGM_I_GOOD], good);
		}
		SGM_SYNC();
		if (lane == 0) {
			const int good = w.isc[SGM_I_GOOD], best = w.isc[SGM_I_BEST];
			w.isc[SGM_I_ITER] = iter + 1;
			if (model && good > (best > 3 ? best : 3)) {
				w.isc[SGM_I_SEL] ^= 1;	/* std::swap(tmask, mask) */
				for (int r = 0; r < 9; r++)
					d[SGM_D_HBEST + r] = d[SGM_D_HCUR + r];
				w.isc[SGM_I_BEST] = good;
				w.isc[SGM_I_NITERS] = sgm_update_num_iters(SGM_RANSAC_CONFIDENCE, (double)(count - good) / count, niters);
			}
		}
		SGM_SYNC();
	}
	if (w.isc[SGM_I_BEST] <= 0)
		return 0;
	/* icvCompressPoints: the inliers' pair indices, in order */
	if (lane == 0) {
		const unsigned char *mk = w.isc[SGM_I_SEL] ? w.tmask : w.mask;
		int n = 0;
		for (int i = 0; i < count; i++)
			if (mk[i])
				w.choice[n++] = i;
		w.isc[SGM_I_NINL] = n;
	}
	SGM_SYNC();
	const int ninl = w.isc[SGM_I_NINL];
	const SgmPoints inl = {&w, w.choice};
	/* runKernel on the inliers; a degenerate set keeps RANSAC's model */
	double *c = d + SGM_D_PREV, *s = c + 4;	/* refine's slots, not yet in use */
	{
		const SgmCentroidTerms fc = {inl};
		sgm_sums<4>(w, lane, nlanes, ninl, fc, d + SGM_D_SUM);
		if (lane == 0)
			for (int k = 0; k < 4; k++)
				c[k] = d[SGM_D_SUM + k] / ninl;
		SGM_SYNC();
		const SgmSpreadTerms fs = {inl, c};
		sgm_sums<4>(w, lane, nlanes, ninl, fs, d + SGM_D_SUM);
		if (lane == 0) {
			for (int k = 0; k < 4; k++)
				s[k] = d[SGM_D_SUM + k];
			w.isc[SGM_I_MODEL] = sgm_kernel_scales(s, ninl);
		}
		SGM_SYNC();
		const int ok = w.isc[SGM_I_MODEL];
		SGM_SYNC();
		if (ok) {
			const SgmLtLTerms fl = {inl, c, s};
			sgm_sums<45>(w, lane, nlanes, ninl, fl, d + SGM_D_SUM);
			if (lane == 0)
				sgm_kernel_finish(c, s, d + SGM_D_SUM, d + SGM_D_HBEST);
			SGM_SYNC();
		}
	}
	sgm_refine(w, lane, nlanes, inl, ninl);
	int nz = 0;
	for (int r = 0; r < 9; r++)
		nz += d[SGM_D_HBEST + r] != 0.0;
	return nz >= 1;
}

/* ---------------------------------------------------------------------------------- a frame */

SGM_HD void sgm_result_clear(sg_starmatch_result *o, int status) {
	o->status = status;
	o->nbpoints = o->nbright = o->scale_retry = o->nwinners = o->npairs = o->nr_recalc = o->inliers = 0;
	o->ransac_iters = o->lm_iters = 0;
	for (int k = 0; k < 6; k++)
		o->trans0[k] = o->trans[k] = 0.0;
	o->sig = o->sx = o->sy = 0.0;
	for (int k = 0; k < 9; k++)
		o->hom[k] = 0.0;
	o->fwhmx = o->fwhmy = 0.f;
	o->shiftx = o->shifty = 0.0;
}

/* new_star_match(A, B, n): A, B are (xpos, ypos, mag) triples, n >= AT_MATCH_MINPAIRS and at most the
 * workspace's nmax.  Lane 0 writes *out (FWHM_average is the caller's) and, if pairs is not NULL,
 * all lanes write pairs [MAX_STARS_FITTED][2] = (A index, B index), -1 padded.  Called by all lanes. */
SGM_HD void sgm_frame(const SgmWork &w, int lane, int nlanes, const double *A, const double *B, int n, sg_starmatch_result *out,
		int32_t *pairs) {
	const int nb = n < AT_MATCH_NBRIGHT ? n : AT_MATCH_NBRIGHT;
	sg_starmatch_result o;
	sgm_result_clear(&o, SG_MATCH_NO_TRANS);
	o.nbpoints = n;
	o.nbright = nb;
	for (int i = lane; i < n; i += nlanes) {
		w.ax[i] = A[3 * (size_t)i];
		w.ay[i] = A[3 * (size_t)i + 1];
		w.bx[i] = B[3 * (size_t)i];
		w.by[i] = B[3 * (size_t)i + 1];
	}
	if (pairs)
		for (int i = lane; i < 2 * MAX_STARS_FITTED; i += nlanes)
			pairs[i] = -1;
	SGM_SYNC();
	sgm_triangles_votes(w, lane, nlanes, A, B, n, nb);
	int found = 0;
	for (int retry = 0; retry < 2 && !found; retry++) {
		sgm_winners(w, lane, nlanes, w.vote + retry * 400, nb);
		found = sgm_iter_trans(w, lane, nlanes, w.isc[SGM_I_NW], 0);
		o.scale_retry = retry;
		SGM_SYNC();
	}
	if (found) {
		for (int k = 0; k < 6; k++)
			o.trans0[k] = w.dsc[SGM_D_TR + k];
		o.nwinners = w.isc[SGM_I_NR];
		SGM_SYNC();
		sgm_match_lists(w, lane, nlanes, n);
		const int np = w.isc[SGM_I_NP];
		o.npairs = np;
		if (pairs)
			for (int i = lane; i < np; i += nlanes) {
				pairs[2 * i] = w.pa[i];
				pairs[2 * i + 1] = w.pb[i];
			}
		/* atCalcRMS, with the TRANS of atFindTrans still in place */
		if (np > 0) {
			SgmRmsTerms f = {&w, 0, 0.0, 0.0};
			sgm_sums<3>(w, lane, nlanes, np, f, w.dsc + SGM_D_SUM);
			f.clip = 1;
			f.xlim = 9 * (w.dsc[SGM_D_SUM] / np);
			f.ylim = 9 * (w.dsc[SGM_D_SUM + 1] / np);
			SGM_SYNC();
			sgm_sums<3>(w, lane, nlanes, np, f, w.dsc + SGM_D_SUM);
			const int left = np - (int)w.dsc[SGM_D_SUM + 2];
			o.sx = w.dsc[SGM_D_SUM] <= 0.0 ? 0.0 : sqrt(w.dsc[SGM_D_SUM] / left);
			o.sy = w.dsc[SGM_D_SUM + 1] <= 0.0 ? 0.0 : sqrt(w.dsc[SGM_D_SUM + 1] / left);
			SGM_SYNC();
		}
		o.status = SG_MATCH_NO_RECALC;
		if (np >= AT_MATCH_STARTN_LINEAR && sgm_iter_trans(w, lane, nlanes, np, 1)) {
			for (int k = 0; k < 6; k++)
				o.trans[k] = w.dsc[SGM_D_TR + k];
			o.nr_recalc = w.isc[SGM_I_NR];
			o.sig = w.dsc[SGM_D_SIG];
			SGM_SYNC();
			o.status = SG_MATCH_NO_HOMOGRAPHY;
		}
	}
	if (o.status == SG_MATCH_NO_HOMOGRAPHY) {
		const int np = o.npairs;
		/* the recalc dropped pairs in place: cvCalculH takes all the matched pairs again */
		sgm_pairs_from_choice(w, lane, nlanes, n);
		const int ok = sgm_homography(w, lane, nlanes, np);
		o.inliers = ok ? w.isc[SGM_I_BEST] : 0;
		o.ransac_iters = w.isc[SGM_I_ITER];
		o.lm_iters = w.isc[SGM_I_LM];
		if (ok) {
			for (int k = 0; k < 9; k++)
				o.hom[k] = w.dsc[SGM_D_HBEST + k];
			o.shiftx = +o.hom[2];
			o.shifty = -o.hom[5];
			o.status = SG_MATCH_OK;
		}
	}
	SGM_SYNC();
	if (lane == 0)
		*out = o;
}

