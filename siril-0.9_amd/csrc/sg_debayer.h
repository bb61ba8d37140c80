/*
 * sg_debayer.h - the per-pixel rules of the CFA demosaicing methods, host + device:
 * bayer_Bilinear (src/algos/demosaicing.c:89-176), bayer_NearestNeighbor (:177-244) and the
 * VNG pass of bayer_VNG (:246-420).
 *
 * All three are written for one output pixel with an accessor for its neighbourhood, so the
 * host readers (sg_io.hip: debayer_area_host) and the kernels (k_debayer_nn, k_debayer_vng)
 * run the same source:
 *   - sg_bilinear_px / sg_nn_px take at(dy, dx) = the CFA sample at (y + dy, x + dx);
 *   - sg_vng_px takes B(dy, dx, c) = colour c of the BILINEAR image at (y + dy, x + dx),
 *     dy, dx in -2..2.  The reference runs VNG in place behind a three-row delay buffer, so
 *     every read sees bilinear values: for an image of at least 6 rows VNG is this pure
 *     function of the 5x5 bilinear neighbourhood on rows 2..H-3, columns 2..W-3, and the
 *     two-pixel ring keeps the bilinear result (tests/debayer_vng_ref.py holds the literal
 *     loop and checks the two forms against each other).
 *
 * The VNG term table is the algorithm's data (64 pairs of positions whose difference feeds
 * the gradients of the directions in `mask`), restated as SgVngTerm entries.  A term counts
 * for a pixel only when both positions have the same CFA colour there and the pair is not a
 * full diagonal step of that colour (:326-332), which depends on the pattern and the pixel's
 * row / column parity alone: sg_vng_px is a template on those three, so each instantiation
 * keeps its surviving terms as straight-line code (`if constexpr`), with no table walk.
 */
#ifndef SG_DEBAYER_H
#define SG_DEBAYER_H

#include <stdint.h>
#include <utility>

#if defined(__HIPCC__)
#define SG_DB_HD __host__ __device__ inline
#else
#define SG_DB_HD inline
#endif

/* CFA colour (0 R, 1 G, 2 B) of site (y, x) under sensor_pattern `pat` (SG_BAYER_*: RGGB,
 * BGGR, GBRG, GRBG); only the parities of y and x count, negative values included (FC(),
 * demosaicing.c:276, with the `filters` words of :299-311) */
SG_DB_HD constexpr int sg_cfa_color(int pat, int y, int x) {
	const bool odd = ((y + x) & 1) != 0;
	if (odd == (pat < 2))
		return 1;
	const int first = (pat == 0 || pat == 3) ? 0 : 2;	/* the red / blue of even rows */
	return (y & 1) ? 2 - first : first;
}

/* bilinear, interior pixels (1 <= y <= H-2, 1 <= x <= W-2; the border stays 0): col = the
 * site's colour, rowc = the red / blue of its row (used at green sites) */
template <class At>
SG_DB_HD void sg_bilinear_px(int col, int rowc, At at, int rgb[3]) {
	const int c = at(0, 0);
	if (col != 1) {
		rgb[col] = c;
		rgb[1] = (at(-1, 0) + at(0, -1) + at(0, 1) + at(1, 0) + 2) >> 2;
		rgb[2 - col] = (at(-1, -1) + at(-1, 1) + at(1, -1) + at(1, 1) + 2) >> 2;
	} else {
		rgb[1] = c;
		rgb[rowc] = (at(0, -1) + at(0, 1) + 1) >> 1;
		rgb[2 - rowc] = (at(-1, 0) + at(1, 0) + 1) >> 1;
	}
}

/* nearest neighbour, pixels y <= H-2, x <= W-2 (the last row and column stay 0): the three
 * colours of the 2x2 cell whose top-left corner the pixel is; a green site takes its green
 * from the diagonal, not from itself */
template <class At>
SG_DB_HD void sg_nn_px(int col, int rowc, At at, int rgb[3]) {
	if (col != 1) {
		rgb[col] = at(0, 0);
		rgb[1] = at(0, 1);
		rgb[2 - col] = at(1, 1);
	} else {
		rgb[1] = at(1, 1);
		rgb[rowc] = at(0, 1);
		rgb[2 - rowc] = at(1, 0);
	}
}

struct SgVngTerm {
	signed char y1, x1, y2, x2, shift;
	unsigned char mask;	/* bit g: the term feeds the gradient of direction g */
};
struct SgVngTable {
	SgVngTerm t[64];
};
SG_DB_HD constexpr SgVngTable sg_vng_table() {
	return SgVngTable{{
		{-2, -2, 0, -1, 0, 0x01}, {-2, -2, 0, 0, 1, 0x01}, {-2, -1, -1, 0, 0, 0x01}, {-2, -1, 0, -1, 0, 0x02},
		{-2, -1, 0, 0, 0, 0x03}, {-2, -1, 0, 1, 1, 0x01}, {-2, 0, 0, -1, 0, 0x06}, {-2, 0, 0, 0, 1, 0x02},
		{-2, 0, 0, 1, 0, 0x03}, {-2, 1, -1, 0, 0, 0x04}, {-2, 1, 0, -1, 1, 0x04}, {-2, 1, 0, 0, 0, 0x06},
		{-2, 1, 0, 1, 0, 0x02}, {-2, 2, 0, 0, 1, 0x04}, {-2, 2, 0, 1, 0, 0x04}, {-1, -2, -1, 0, 0, 0x80},
		{-1, -2, 0, -1, 0, 0x01}, {-1, -2, 1, -1, 0, 0x01}, {-1, -2, 1, 0, 1, 0x01}, {-1, -1, -1, 1, 0, 0x88},
		{-1, -1, 1, -2, 0, 0x40}, {-1, -1, 1, -1, 0, 0x22}, {-1, -1, 1, 0, 0, 0x33}, {-1, -1, 1, 1, 1, 0x11},
		{-1, 0, -1, 2, 0, 0x08}, {-1, 0, 0, -1, 0, 0x44}, {-1, 0, 0, 1, 0, 0x11}, {-1, 0, 1, -2, 1, 0x40},
		{-1, 0, 1, -1, 0, 0x66}, {-1, 0, 1, 0, 1, 0x22}, {-1, 0, 1, 1, 0, 0x33}, {-1, 0, 1, 2, 1, 0x10},
		{-1, 1, 1, -1, 1, 0x44}, {-1, 1, 1, 0, 0, 0x66}, {-1, 1, 1, 1, 0, 0x22}, {-1, 1, 1, 2, 0, 0x10},
		{-1, 2, 0, 1, 0, 0x04}, {-1, 2, 1, 0, 1, 0x04}, {-1, 2, 1, 1, 0, 0x04}, {0, -2, 0, 0, 1, 0x80},
		{0, -1, 0, 1, 1, 0x88}, {0, -1, 1, -2, 0, 0x40}, {0, -1, 1, 0, 0, 0x11}, {0, -1, 2, -2, 0, 0x40},
		{0, -1, 2, -1, 0, 0x20}, {0, -1, 2, 0, 0, 0x30}, {0, -1, 2, 1, 1, 0x10}, {0, 0, 0, 2, 1, 0x08},
		{0, 0, 2, -2, 1, 0x40}, {0, 0, 2, -1, 0, 0x60}, {0, 0, 2, 0, 1, 0x20}, {0, 0, 2, 1, 0, 0x30},
		{0, 0, 2, 2, 1, 0x10}, {0, 1, 1, 0, 0, 0x44}, {0, 1, 1, 2, 0, 0x10}, {0, 1, 2, -1, 1, 0x40},
		{0, 1, 2, 0, 0, 0x60}, {0, 1, 2, 1, 0, 0x20}, {0, 1, 2, 2, 0, 0x10}, {1, -2, 1, 0, 0, 0x80},
		{1, -1, 1, 1, 0, 0x88}, {1, 0, 1, 2, 0, 0x08}, {1, 0, 2, -1, 0, 0x40}, {1, 0, 2, 1, 0, 0x10},
	}};
}
/* the eight directions, clockwise from the upper left (:269-270) */
SG_DB_HD constexpr int sg_vng_dir_y(int g) {
	return g < 3 ? -1 : (g == 3 || g == 7) ? 0 : 1;
}
SG_DB_HD constexpr int sg_vng_dir_x(int g) {
	return (g == 0 || g >= 6) ? -1 : (g == 1 || g == 5) ? 0 : 1;
}

/* does term T count at a pixel of parity (PY, PX) under pattern PAT (:326-332) */
SG_DB_HD constexpr bool sg_vng_term_on(int pat, int py, int px, int T) {
	const SgVngTerm t = sg_vng_table().t[T];
	const int color = sg_cfa_color(pat, py + t.y1, px + t.x1);
	if (sg_cfa_color(pat, py + t.y2, px + t.x2) != color)
		return false;
	const int diag = (sg_cfa_color(pat, py, px + 1) == color && sg_cfa_color(pat, py + 1, px) == color) ? 2 : 1;
	const int ay = t.y1 > t.y2 ? t.y1 - t.y2 : t.y2 - t.y1, ax = t.x1 > t.x2 ? t.x1 - t.x2 : t.x2 - t.x1;
	return !(ay == diag && ax == diag);
}

template <int PAT, int PY, int PX, int T, class Bil>
SG_DB_HD void sg_vng_term(const Bil &B, int (&gval)[8]) {
	if constexpr (sg_vng_term_on(PAT, PY, PX, T)) {
		constexpr SgVngTerm t = sg_vng_table().t[T];
		constexpr int color = sg_cfa_color(PAT, PY + t.y1, PX + t.x1);
		int diff = B(t.y1, t.x1, color) - B(t.y2, t.x2, color);
		diff = (diff < 0 ? -diff : diff) << t.shift;
		if constexpr ((t.mask & 0x01) != 0) gval[0] += diff;
		if constexpr ((t.mask & 0x02) != 0) gval[1] += diff;
		if constexpr ((t.mask & 0x04) != 0) gval[2] += diff;
		if constexpr ((t.mask & 0x08) != 0) gval[3] += diff;
		if constexpr ((t.mask & 0x10) != 0) gval[4] += diff;
		if constexpr ((t.mask & 0x20) != 0) gval[5] += diff;
		if constexpr ((t.mask & 0x40) != 0) gval[6] += diff;
		if constexpr ((t.mask & 0x80) != 0) gval[7] += diff;
	}
}
template <int PAT, int PY, int PX, class Bil, int... T>
SG_DB_HD void sg_vng_gradients(const Bil &B, int (&gval)[8], std::integer_sequence<int, T...>) {
	(sg_vng_term<PAT, PY, PX, T>(B, gval), ...);
}

/* direction G's share of the average (:389-398): the neighbour's colours, but for the centre's
 * own colour, where the neighbour is of another colour, the mean of the centre and the sample
 * two steps away */
template <int PAT, int PY, int PX, int G, class Bil>
SG_DB_HD void sg_vng_take(const Bil &B, const int (&gval)[8], int thold, int (&sum)[3], int &num) {
	constexpr int y = sg_vng_dir_y(G), x = sg_vng_dir_x(G);
	constexpr int color = sg_cfa_color(PAT, PY, PX);
	constexpr bool half = sg_cfa_color(PAT, PY + y, PX + x) != color && sg_cfa_color(PAT, PY + 2 * y, PX + 2 * x) == color;
	if (gval[G] <= thold) {
		for (int c = 0; c < 3; c++)
			if (c == color && half)
				sum[c] += (B(0, 0, c) + B(2 * y, 2 * x, color)) >> 1;
			else
				sum[c] += B(y, x, c);
		num++;
	}
}
template <int PAT, int PY, int PX, class Bil, int... G>
SG_DB_HD void sg_vng_average(const Bil &B, const int (&gval)[8], int thold, int (&sum)[3], int &num,
		std::integer_sequence<int, G...>) {
	(sg_vng_take<PAT, PY, PX, G>(B, gval, thold, sum, num), ...);
}

/* VNG of one pixel of parity (PY, PX): rgb[] = round_to_WORD of the centre's own sample plus the
 * mean colour difference over the directions whose gradient is at most gmin + gmax / 2; the
 * bilinear pixel where every gradient is 0 (:359-405) */
template <int PAT, int PY, int PX, class Bil>
SG_DB_HD void sg_vng_px(const Bil &B, int rgb[3]) {
	int gval[8] = {0, 0, 0, 0, 0, 0, 0, 0};
	sg_vng_gradients<PAT, PY, PX>(B, gval, std::make_integer_sequence<int, 64>());
	int gmin = gval[0], gmax = gval[0];
	for (int g = 1; g < 8; g++) {
		gmin = gval[g] < gmin ? gval[g] : gmin;
		gmax = gval[g] > gmax ? gval[g] : gmax;
	}
	if (gmax == 0) {
		for (int c = 0; c < 3; c++)
			rgb[c] = B(0, 0, c);
		return;
	}
	const int thold = gmin + (gmax >> 1);
	int sum[3] = {0, 0, 0}, num = 0;
	sg_vng_average<PAT, PY, PX>(B, gval, thold, sum, num, std::make_integer_sequence<int, 8>());
	constexpr int color = sg_cfa_color(PAT, PY, PX);
	const int own = B(0, 0, color);
	for (int c = 0; c < 3; c++) {
		int t = own;
		if (c != color)
			t += (sum[c] - sum[color]) / num;	/* C division: toward zero */
		rgb[c] = t < 0 ? 0 : t > 65535 ? 65535 : t;
	}
}

/* sg_vng_px for a run-time pattern and pixel position (the host readers) */
template <class Bil>
SG_DB_HD void sg_vng_px_any(int pat, int y, int x, const Bil &B, int rgb[3]) {
	switch (pat * 4 + (y & 1) * 2 + (x & 1)) {
#define SG_VNG_CASE(P, Y, X) \
	case (P) * 4 + (Y) * 2 + (X): \
		sg_vng_px<P, Y, X>(B, rgb); \
		break;
#define SG_VNG_PAT(P) SG_VNG_CASE(P, 0, 0) SG_VNG_CASE(P, 0, 1) SG_VNG_CASE(P, 1, 0) SG_VNG_CASE(P, 1, 1)
		SG_VNG_PAT(0) SG_VNG_PAT(1) SG_VNG_PAT(2) SG_VNG_PAT(3)
#undef SG_VNG_PAT
#undef SG_VNG_CASE
	default:
		break;
	}
}

#endif /* SG_DEBAYER_H */
