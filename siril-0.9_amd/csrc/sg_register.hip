/*
 * sg_register.hip - gfx950 DFT registration (replaces register_shift_dft,
 * src/registration/registration.c:182-400) and the planetary quality estimate it records
 * (QualityEstimate, src/algos/quality.c:46-349; normalizeQualityData registration.c:163-176).
 *
 * Per frame the reference computes, with FFTW in complex double,
 *     c = IFFT2( FFT2(ref) * conj(FFT2(img)) )      (unnormalised, FFTW_BACKWARD)
 * and takes the first strict maximum of creal(c) in row-major order (:337-351).  Here:
 *   - frames go through the 2-D FFT two at a time, packed as a + i b (both are real), and
 *     their spectra are separated with F_a(k) = (Z(k) + conj Z(-k))/2,
 *     F_b(k) = (Z(k) - conj Z(-k))/2i;
 *   - the two cross-power spectra are packed back as P = R conj F_a + i R conj F_b, whose
 *     inverse is c_a + i c_b (both correlations are real): one forward and one inverse
 *     complex 2-D FFT per PAIR of frames;
 *   - power-of-two sides: Stockham passes of radix 8 (then 4 / 2) in LDS on half spectra
 *     (rows: one workgroup per row; columns: one workgroup per strip of CW columns), in fp32
 *     by default, fp64 for the pairs re-run below (SG_REG_FP=64: fp64 throughout), twiddles
 *     from host tables; any other side: mixed radix 8/4/2/3/5/7, or Bluestein's chirp-z for
 *     a prime factor above 7, with transposed column passes, in fp64;
 *   - the inverse row pass fuses a per-row TOP-2 arg-max (first index on ties), a tiny kernel
 *     reduces the rows in order.
 * Near ties: a maximum is decided where it beats the runner-up by more than the pass's error
 * bound, 2^-15 S^2 ||ref|| ||img|| in fp32 (the pair then re-runs in fp64) and 2^-32 in fp64
 * (far above fp64 FFT rounding: every index within it is listed and its exact integer
 * correlation computed; the largest wins, the lowest index among exact equals).  So shifts
 * equal the reference wherever FFTW's rounding does not decide between exactly equal
 * correlations (FFTW's choice there is unspecified: "parity unpinned").
 */
#include "sg_common.hpp"
#include "sg_ctx.hpp"
#include "sg_fft.hpp"
#include <math.h>
#include <stdlib.h>
#include <string.h>
#include <algorithm>
#include <thread>
#include <type_traits>
#include <vector>

/* strip of workgroup `id` out of n: the dispatcher deals workgroups round-robin over the 8
 * XCDs, so neighbouring strips (which share 128-B lines: a strip row is 64 B) would be
 * fetched by two L2s; give each XCD a contiguous range of strips instead (PMC FETCH_SIZE
 * of the column passes halves) */
__device__ __forceinline__ int sg_xcd_strip(int id, int n) {
	if (n & 7)
		return id;
	return (id & 7) * (n >> 3) + (id >> 3);
}

/* column pass (forward or inverse) over strips of CW adjacent columns */
template <class C, int EPT = 8>
__global__ void __launch_bounds__(1024)
k_reg_cols(C *__restrict__ work, int S, int logS, int CW, const C *__restrict__ tw, int inverse) {
	extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
	C *buf = (C *)smem;
	const int x0 = sg_xcd_strip(blockIdx.x, gridDim.x) * CW, pair = blockIdx.y;
	const int bstride = sg_col_stride<C>(S);
	C *base = work + (size_t)pair * S * S + x0;
	(void)logS;
	sg_fft_io<false, EPT>(buf, S, CW, bstride, tw, inverse != 0, [&](int c, int r) { return base[(size_t)r * S + c]; },
			[&](int c, int r, C v) { base[(size_t)r * S + c] = v; });
}

/* one term of the packed cross-power spectrum at (ky, kx): zk = Z(ky, kx),
 * zm = Z(-ky, -kx), rk = R(ky, kx).  F_a = (zk + conj zm) / 2, F_b = (zk - conj zm) / 2i;
 * result R conj F_a + i R conj F_b.  The term at (-ky, -kx) is this function with zk and
 * zm swapped (the negated differences are exact, products and sums commute), so every
 * element is formed by the same expression. */
__device__ __forceinline__ sg_c64 sg_xpower_at(sg_c64 zk, sg_c64 zm, sg_c64 rk) {
	const double ar = 0.5 * (zk.x + zm.x), ai = 0.5 * (zk.y - zm.y);
	const double br = 0.5 * (zk.y + zm.y), bi = -0.5 * (zk.x - zm.x);
	const double pr = rk.x * ar + rk.y * ai, pi = rk.y * ar - rk.x * ai;
	const double qr = rk.x * br + rk.y * bi, qi = rk.y * br - rk.x * bi;
	return make_double2(pr - qi, pi + qr);
}

/* ---------------------------------------------------------------------------------------
 * Half-spectrum pass order (default): three plane passes per pair instead of four.
 *   1. k_reg_rows_fwd_half: row FFT of a + i b, separated per row into the row spectra of
 *      the two real frames, A(kx) = (z(kx) + conj z(-kx))/2, B(kx) = (z(kx) - conj z(-kx))/2i,
 *      of which kx in [0, S/2] is kept (Hermitian rows).  A(0) and A(S/2) are real, so
 *      column 0 packs A(0) + i A(S/2).  Layout of a pair plane row: [A' | B'], S/2 + S/2.
 *   2. k_reg_cols_xpower: per column (of A' or B'), forward column FFT, cross-power with
 *      the reference's column (R conj F), inverse column FFT: the cross-power needs no
 *      mirrored column any more, so the forward and inverse column passes fuse.  Column 0
 *      of each half holds two real sequences and is separated / re-packed over (ky, -ky),
 *      which lie in the same column.
 *   3. k_reg_rows_inv_half_argmax: the inverse column output is Hermitian in kx (the
 *      correlation is real), so each row's full spectrum is rebuilt from kx <= S/2, the
 *      two frames packed as Qa + i Qb, inverse row FFT -> c_a + i c_b, arg-max fused.
 * Same unnormalised FFTW_BACKWARD result as the full complex transforms; plane traffic per
 * pair 84 B per pixel instead of 116.
 * ------------------------------------------------------------------------------------- */
/* the frames' selections as the registration kernels read them: selection f, row r at
 * p[f fp + r rp] (elements).  Contiguous S x S selections: fp = S S, rp = S; in place in resident
 * frames (sg_register_dft_u16_device_pitched): the frames' plane / row pitches */
struct SgSel {
	const uint16_t *p;
	long long fp, rp;
	__device__ __forceinline__ const uint16_t *frame(int f) const { return p + (size_t)f * (size_t)fp; }
};

#ifndef SG_REG_FWD_WPE
#define SG_REG_FWD_WPE 4	/* forward row pass: waves per SIMD its register budget is sized for (4: 127 VGPRs, 28 B of scratch, registration 5.93 -> 5.82 ms on configs[1]; 1: 134 VGPRs; 6: 208 B of scratch, 6.97 ms) */
#endif
template <class C>
__global__ void __launch_bounds__(512) __attribute__((amdgpu_waves_per_eu(SG_REG_FWD_WPE)))
k_reg_rows_fwd_half(SgSel sel, const int *__restrict__ fa, const int *__restrict__ fb,
		int S, const C *__restrict__ tw, C *__restrict__ work, unsigned long long *__restrict__ energy, int rpb) {
	typedef typename SgReal<C>::T T;
	extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
	C *buf = (C *)smem;
	const int pair = blockIdx.y, H = S >> 1, per = S >> 3;
	const size_t plane = (size_t)S * S;
	const uint16_t *pa = sel.frame(fa[pair]);
	const int b = fb[pair];
	const uint16_t *pb = b >= 0 ? sel.frame(b) : nullptr;
	/* rpb rows per workgroup; the next row's samples are loaded into registers before this
	 * row's transform (the first pass's inputs: thread t takes elements t + r S / 8), so its
	 * load latency hides behind the LDS passes instead of opening every row (round 2: one row
	 * per workgroup, 1.75 ms per 64 pairs of 2048^2 at 1.8 TB/s) */
	const int t = threadIdx.x;
	const bool act = t < per;
	uint32_t ra[8], rb[8];
	auto fetch = [&](int row) {
#pragma unroll
		for (int r = 0; r < 8; r++) {
			const size_t i = (size_t)row * sel.rp + (size_t)(t + r * per);
			ra[r] = act ? (uint32_t)pa[i] : 0u;
			rb[r] = (act && pb) ? (uint32_t)pb[i] : 0u;
		}
	};
	unsigned long long ea = 0, eb = 0;
	const int row0 = blockIdx.x * rpb;
	fetch(row0);
	for (int k = 0; k < rpb; k++) {
		const int row = row0 + k;
		C v[1][8];
#pragma unroll
		for (int r = 0; r < 8; r++) {
			v[0][r] = sg_mk<C>((T)ra[r], (T)rb[r]);
			ea += (unsigned long long)(ra[r] * ra[r]);
			eb += (unsigned long long)(rb[r] * rb[r]);
		}
		if (k + 1 < rpb)
			fetch(row + 1);
		if (k > 0)
			__syncthreads();	/* the previous row's separation has read buf */
		sg_fft_io_regs<8>(buf, S, 1, S, tw, false, v, [&](int, int i, C val) { buf[sg_pad(i)] = val; });
		__syncthreads();
		C *out = work + (size_t)pair * plane + (size_t)row * S;
		for (int kx = threadIdx.x; kx < H; kx += blockDim.x) {
			const C zk = buf[sg_pad(kx)], zm = buf[sg_pad(kx ? S - kx : H)];
			C A, B;
			if (kx == 0) {
				A = sg_mk<C>(zk.x, zm.x);	/* A(0) + i A(S/2) */
				B = sg_mk<C>(zk.y, zm.y);
			} else {
				A = sg_mk<C>((T)0.5 * (zk.x + zm.x), (T)0.5 * (zk.y - zm.y));
				B = sg_mk<C>((T)0.5 * (zk.y + zm.y), (T)-0.5 * (zk.x - zm.x));
			}
			out[kx] = A;
			out[H + kx] = B;
		}
	}
	sg_energy_add(ea, eb, fa[pair], b, energy);
}

/* R conj F */
template <class C>
__device__ __forceinline__ C sg_rconj(C r, C f) {
	return sg_mk<C>(r.x * f.x + r.y * f.y, r.y * f.x - r.x * f.y);
}

/* The reference-spectrum loads of all 8 cross-power items of a thread are issued together
 * (launches are sized so that CW * S = 8 * blockDim, thr_for).  Issuing them before the
 * forward FFT instead spills (128 VGPRs at 4 waves per SIMD). */
template <class C, int EPT = 8, int WPE = 1>
__global__ void __launch_bounds__(1024) __attribute__((amdgpu_waves_per_eu(WPE)))
k_reg_cols_xpower(C *__restrict__ work, const C *__restrict__ spec, int S, int CW,
		const C *__restrict__ tw) {
	extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
	C *buf = (C *)smem;
	const int x0 = sg_xcd_strip(blockIdx.x, gridDim.x) * CW, pair = blockIdx.y;
	typedef typename SgReal<C>::T T;
	const int bstride = sg_col_stride<C>(S), H = S >> 1;
	C *base = work + (size_t)pair * S * S + x0;
	auto slot = [&](int c, int r) -> C & { return buf[(size_t)c * bstride + sg_pad(r)]; };
	constexpr int NI = EPT;
	const int items = CW * S, lcw = sg_log2(CW);	/* CW: a power of two */
	/* the reference's packed column 0 (a strip starting at kx = 0 of either half) also needs
	 * R(-ky): read where it is used, so the other strips keep no second register array */
	C rk[NI];
	auto fetch = [&]() {
#pragma unroll
		for (int it = 0; it < NI; it++) {
			const int t = threadIdx.x + it * blockDim.x;
			rk[it] = sg_mk<C>((T)0, (T)0);
			if (t < items) {
				const int c = t & (CW - 1), ky = t >> lcw, kx = (x0 + c) & (H - 1);
				rk[it] = spec[(size_t)ky * S + kx];
			}
		}
	};
	sg_fft_io<false, EPT>(buf, S, CW, bstride, tw, false, [&](int c, int r) { return base[(size_t)r * S + c]; },
			[&](int c, int r, C v) { slot(c, r) = v; });
	fetch();
	__syncthreads();
#pragma unroll
	for (int it = 0; it < NI; it++) {
		const int t = threadIdx.x + it * blockDim.x;
		if (t >= items)
			continue;
		const int c = t & (CW - 1), ky = t >> lcw, kx = (x0 + c) & (H - 1);
		if (kx) {
			slot(c, ky) = sg_rconj(rk[it], slot(c, ky));
			continue;
		}
		/* packed column: Z = F0 + i FN (F0, FN spectra of real columns), same for the
		 * reference; P = R0 conj F0 + i RN conj FN, written at ky and -ky */
		const int m = (S - ky) & (S - 1);
		if (m < ky)
			continue;
		const C zk = slot(c, ky), zm = slot(c, m), r1 = rk[it], r2 = spec[(size_t)m * S];
		const C f0 = sg_mk<C>((T)0.5 * (zk.x + zm.x), (T)0.5 * (zk.y - zm.y));
		const C fn = sg_mk<C>((T)0.5 * (zk.y + zm.y), (T)-0.5 * (zk.x - zm.x));
		const C r0 = sg_mk<C>((T)0.5 * (r1.x + r2.x), (T)0.5 * (r1.y - r2.y));
		const C rn = sg_mk<C>((T)0.5 * (r1.y + r2.y), (T)-0.5 * (r1.x - r2.x));
		const C p0 = sg_rconj(r0, f0), pn = sg_rconj(rn, fn);
		slot(c, ky) = sg_mk<C>(p0.x - pn.y, p0.y + pn.x);
		if (m != ky)	/* P0(-k) = conj P0(k), PN(-k) = conj PN(k) */
			slot(c, m) = sg_mk<C>(p0.x + pn.y, pn.x - p0.y);
	}
	__syncthreads();
	sg_fft_io<true, EPT>(buf, S, CW, bstride, tw, true, [&](int c, int r) { return slot(c, r); },
			[&](int c, int r, C v) { base[(size_t)r * S + c] = v; });
}

/* ---------------------------------------------------------------------------------------
 * Wave-level fused column pass, fp32, S = 2048 (configs[1] / configs[4]): one WAVE per column
 * of an 8-column strip, the 2048-point transforms as 32 x 64 four-step FFTs held in registers
 * (32 complex per lane), so the block synchronises only around the coalesced strip load and
 * store.  Forward: lane l holds x[64 j + l] (j = 0..31); a 32-point DFT over j in registers,
 * twiddles w_S^(l k1), a transpose through the wave's own LDS column (rows of 66 for banks) to
 * lane m = (k1 = m / 2, h = m % 2) holding the odd / even lanes' values (i -> l = 2 i + h), a
 * 32-point DFT over i, twiddles w_64^(h k2) and one radix-2 step across the lane pair (DPP):
 * lane m, register k2 then holds X[ky], ky = m / 2 + 32 k2 + 1024 (m % 2).  The cross power is
 * elementwise at ky (the packed column 0 also reads Z(-ky), through the wave's LDS), and the
 * inverse runs the same steps mirrored, ending in natural order.  Same products and packing as
 * k_reg_cols_xpower; the FFT's rounding differs and stays within the fp32 tie tolerance
 * (sg_reg_tol).  The round-3 kernel (1024 threads, four radix-8/4 LDS passes each way) spent
 * ~15 k wave-instructions per column, mostly index arithmetic, LDS traffic and barriers.
 * ------------------------------------------------------------------------------------- */
typedef float sg_v2f __attribute__((ext_vector_type(2)));
__device__ __forceinline__ float2 sg_cmulf(float2 a, float2 b) {
	const sg_v2f av = sg_v2f{a.x, a.y}, bv = sg_v2f{b.x, b.y};
	sg_v2f r;
	asm("v_pk_mul_f32 %0, %1, %2 op_sel_hi:[0,1]\n\t"
	    "v_pk_fma_f32 %0, %1, %2, %0 op_sel:[1,1,0] op_sel_hi:[1,0,1] neg_lo:[1,0,0]"
	    : "=&v"(r) : "v"(av), "v"(bv));
	return make_float2(r.x, r.y);
}
/* the same with a uniform w (a constant root: an SGPR pair, no per-use VGPR moves) */
__device__ __forceinline__ float2 sg_cmulk(float2 a, sg_v2f w) {
	const sg_v2f av = sg_v2f{a.x, a.y};
	sg_v2f r;
	asm("v_pk_mul_f32 %0, %1, %2 op_sel_hi:[0,1]\n\t"
	    "v_pk_fma_f32 %0, %1, %2, %0 op_sel:[1,1,0] op_sel_hi:[1,0,1] neg_lo:[1,0,0]"
	    : "=&v"(r) : "v"(av), "s"(w));
	return make_float2(r.x, r.y);
}

/* s v + o for a per-lane sign s = (+-1, +-1) (the lane pair's radix-2: v + o or o - v, exact) */
__device__ __forceinline__ float2 sg_pm_add(float2 v, float2 o, sg_v2f s2) {
	sg_v2f r;
	asm("v_pk_fma_f32 %0, %1, %2, %3" : "=v"(r) : "v"(s2), "v"(sg_v2f{v.x, v.y}), "v"(sg_v2f{o.x, o.y}));
	return make_float2(r.x, r.y);
}
/* r conj(f) (the cross power's product) */
__device__ __forceinline__ float2 sg_rconjf(float2 r, float2 f) {
	sg_v2f d;
	asm("v_pk_mul_f32 %0, %1, %2 op_sel_hi:[0,1]\n\t"
	    "v_pk_fma_f32 %0, %1, %2, %0 op_sel:[1,1,0] op_sel_hi:[1,0,1] neg_hi:[0,0,1]"
	    : "=&v"(d) : "v"(sg_v2f{r.x, r.y}), "v"(sg_v2f{f.x, f.y}));
	return make_float2(d.x, d.y);
}

/* 32-point DFT of v (natural order in and out) in registers, radix-2 decimation in frequency */
/* d times -i (forward) / +i (inverse), exact: one packed multiply by (1, -1) / (-1, 1) with the
 * halves swapped */
template <bool INV>
__device__ __forceinline__ sg_v2f sg_rot_i(sg_v2f d) {
	sg_v2f r;
	asm("v_pk_mul_f32 %0, %1, %2 op_sel:[1,0] op_sel_hi:[0,1]" : "=v"(r) : "v"(d), "s"(INV ? sg_v2f{-1.0f, 1.0f} : sg_v2f{1.0f, -1.0f}));
	return r;
}
__device__ __forceinline__ sg_v2f sg_cmulk2(sg_v2f a, sg_v2f w) {
	sg_v2f r;
	asm("v_pk_mul_f32 %0, %1, %2 op_sel_hi:[0,1]\n\t"
	    "v_pk_fma_f32 %0, %1, %2, %0 op_sel:[1,1,0] op_sel_hi:[1,0,1] neg_lo:[1,0,0]"
	    : "=&v"(r) : "v"(a), "s"(w));
	return r;
}

/* 32-point DFT of v (natural order in and out) in registers, radix-2 decimation in frequency;
 * each complex value one packed register pair (v_pk_add / v_pk_mul + v_pk_fma per butterfly) */
template <bool INV>
__device__ __forceinline__ void sg_dft32_lane(float2 (&v)[32]) {
	constexpr float C[16] = {1.0f, 0.9807852506637573f, 0.9238795042037964f, 0.8314695954322815f,
		0.7071067690849304f, 0.5555702447891235f, 0.3826834261417389f, 0.19509032368659973f, 0.0f,
		-0.19509032368659973f, -0.3826834261417389f, -0.5555702447891235f, -0.7071067690849304f,
		-0.8314695954322815f, -0.9238795042037964f, -0.9807852506637573f};
	constexpr float SN[16] = {0.0f, 0.19509032368659973f, 0.3826834261417389f, 0.5555702447891235f,
		0.7071067690849304f, 0.8314695954322815f, 0.9238795042037964f, 0.9807852506637573f, 1.0f,
		0.9807852506637573f, 0.9238795042037964f, 0.8314695954322815f, 0.7071067690849304f,
		0.5555702447891235f, 0.3826834261417389f, 0.19509032368659973f};
	sg_v2f x[32];
#pragma unroll
	for (int k = 0; k < 32; k++)
		x[k] = sg_v2f{v[k].x, v[k].y};
#pragma unroll
	for (int half = 16; half >= 1; half >>= 1) {
#pragma unroll
		for (int blk = 0; blk < 32; blk += 2 * half) {
#pragma unroll
			for (int i = 0; i < half; i++) {
				const sg_v2f a = x[blk + i], b = x[blk + i + half];
				x[blk + i] = a + b;
				const sg_v2f d = a - b;
				const int m = i * (16 / half);	/* w_32^m, m < 16 */
				if (m == 0)
					x[blk + i + half] = d;
				else if (m == 8)
					x[blk + i + half] = sg_rot_i<INV>(d);
				else
					x[blk + i + half] = sg_cmulk2(d, sg_v2f{C[m], INV ? SN[m] : -SN[m]});
			}
		}
		__builtin_amdgcn_sched_barrier(0);	/* stage by stage: interleaved stages took 249 VGPRs */
	}
#pragma unroll
	for (int k = 0; k < 32; k++) {
		const sg_v2f t = x[(int)(__builtin_bitreverse32((unsigned)k) >> 27)];
		v[k] = make_float2(t.x, t.y);
	}
}

/* the lane-pair partner's value (lane ^ 1), DPP quad_perm [1, 0, 3, 2] */
__device__ __forceinline__ float2 sg_pair_swap(float2 v) {
	return make_float2(__int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(v.x), 0xB1, 0xF, 0xF, false)),
			__int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(v.y), 0xB1, 0xF, 0xF, false)));
}

/* v[k1] *= w^(lane k1) (k1 >= 1; tw: the forward or inverse table of S entries).  The table is
 * read at k1 = 1, 8, 16, 24 only (lane-scattered loads, 64 distinct lines per instruction, were
 * the pass's bottleneck: 31 of them per transform) and the powers in between are formed by
 * multiplying by w^lane: at most 7 products per twiddle, within the fp32 tie tolerance */
__device__ __forceinline__ void sg_twiddle_rows(float2 (&v)[32], const float2 *__restrict__ tw, int lane) {
	const float2 b = tw[lane];
	float2 t8[3];
#pragma unroll
	for (int q = 0; q < 3; q++)
		t8[q] = tw[lane * 8 * (q + 1)];
	float2 t = b;
#pragma unroll
	for (int k1 = 1; k1 < 32; k1++) {
		if (k1 > 1)
			t = (k1 & 7) ? sg_cmulf(t, b) : t8[(k1 >> 3) - 1];
		v[k1] = sg_cmulf(v[k1], t);
	}
}

/* 2048-point DFT of the wave's line, four-step 32 x 64: lane l holds x[64 j + l] in v[j]; on
 * return lane m holds X[m / 2 + 32 k + 1024 (m % 2)] in v[k] (INV: conjugate roots, the
 * unnormalised inverse).  col: the wave's LDS (32 rows of 66 float2).  tw: the forward table
 * (tw + 2048 is the inverse one). */
template <bool INV>
__device__ __forceinline__ void sg_fft2048_wave(float2 (&v)[32], float2 *col, const float2 *__restrict__ tw, int lane) {
	constexpr int S = 2048, P = 32, TR = 66;
	const float2 *twd = INV ? tw + S : tw;
	sg_dft32_lane<INV>(v);
	sg_twiddle_rows(v, twd, lane);
	__builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
#pragma unroll
	for (int k1 = 0; k1 < P; k1++)
		col[k1 * TR + lane] = v[k1];
	__builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
	const int km = lane >> 1, hm = lane & 1;
#pragma unroll
	for (int i = 0; i < P; i++)
		v[i] = col[km * TR + 2 * i + hm];
	sg_dft32_lane<INV>(v);
	if (hm) {	/* odd lanes: the radix-2 stage's twiddles (uniform loads, SGPR operands) */
#pragma unroll
		for (int k = 1; k < P; k++) {
			const float2 t = twd[32 * k];
			v[k] = sg_cmulk(v[k], sg_v2f{t.x, t.y});
		}
	}
	const float sg1 = hm ? -1.0f : 1.0f;
	const sg_v2f s2 = sg_v2f{sg1, sg1};
#pragma unroll
	for (int k = 0; k < P; k++)
		v[k] = sg_pm_add(v[k], sg_pair_swap(v[k]), s2);
}

#ifndef SG_WCOL_WPE
#define SG_WCOL_WPE 2
#endif
/* physical LDS row of strip row r in column c of a CW-column strip, so that the strip's 8-byte
 * stores (32 banks, 16-lane groups) and its 8-byte reads (64 banks, 32-lane groups, CS = 8 mod 32)
 * are both conflict-free (a 2-way conflict on the stores was 20 % of the column pass's LDS
 * cycles).  CW = 4: a store group is 4 rows x 4 columns, columns 2, 3 XOR the row with 4; CW = 8:
 * 2 rows x 8 columns, column c XORs it with 2 (c / 2). */
template <int CW = 4>
__device__ __forceinline__ int sg_strip_row(int r, int c) {
	return CW == 8 ? r ^ ((c >> 1) << 1) : r ^ ((c >> 1) << 2);
}
/* specp: the reference spectrum in the column pass's lane order, specp[(kx 32 + k) 64 + 2 km + hm]
 * = spec[ky][kx] at ky = km + 32 k + 1024 hm (kx < S / 2), so that the pass reads its reference
 * column with one coalesced 512-B load per k (issued before its forward transform) instead of
 * staging a strip through LDS between two block barriers. */
/* the reference spectrum's forward column pass at S = 2048, wave-level (k_reg_cols_xpower_w's
 * strip staging and transform): columns [0, S/2) of the row-transformed reference plane, written
 * straight into specp's lane order (coalesced 512-B stores), and column 0 also back in natural
 * order (the packed column's wave reads it by ky).  Replaces k_reg_cols + k_spec_perm on the
 * wave-level path (one workgroup per CU there, 0.39 ms beside the pairs' forward rows). */
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(SG_WCOL_WPE)))
k_reg_cols_fwd_perm_w(float2 *__restrict__ spec, float2 *__restrict__ specp, const float2 *__restrict__ tw) {
	constexpr int S = 2048, P = 32, CS = SG_WCOL_CS;
	extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
	float2 *lds = (float2 *)smem;
	const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
	const int x0 = blockIdx.x * 4;
	float2 *col = lds + wave * CS;
	const int sw = sg_strip_row<4>(0, wave);	/* sg_strip_row of this wave's column: lane ^ sw */
#pragma unroll
	for (int it = 0; it < P; it++) {
		const int r = (threadIdx.x >> 2) + 64 * it, c = threadIdx.x & 3;
		lds[c * CS + sg_strip_row(r, c)] = spec[(size_t)r * S + x0 + c];
	}
	__syncthreads();
	float2 v[P];
#pragma unroll
	for (int j = 0; j < P; j++)
		v[j] = col[64 * j + (lane ^ sw)];
	sg_fft2048_wave<false>(v, col, tw, lane);
	const int kx = x0 + wave, km = lane >> 1, hm = lane & 1;
	float2 *sp = specp + (size_t)kx * S;
#pragma unroll
	for (int k = 0; k < P; k++)
		sp[64 * k + lane] = v[k];
	if (kx == 0) {
#pragma unroll
		for (int k = 0; k < P; k++)
			spec[(size_t)(km + 32 * k + 1024 * hm) * S] = v[k];
	}
}

__global__ void __launch_bounds__(64 * 8) __attribute__((amdgpu_waves_per_eu(SG_WCOL_WPE)))
k_reg_cols_xpower_w(float2 *__restrict__ work, const float2 *__restrict__ spec, const float2 *__restrict__ specp,
		const float2 *__restrict__ tw) {
	constexpr int S = 2048, H = 1024, P = 32, CW = 8, CS = SG_WCOL_CS, TR = 66;
	extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
	float2 *lds = (float2 *)smem;
	const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
	const int x0 = sg_xcd_strip(blockIdx.x, gridDim.x) * CW, pair = blockIdx.y;
	float2 *base = work + (size_t)pair * S * S + x0;
	float2 *col = lds + wave * CS;
	const int sw = sg_strip_row<CW>(0, wave);	/* sg_strip_row of this wave's column: lane ^ sw */
	auto wsync = [] { __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront"); };
	/* strip -> LDS: rows of 8 columns (64 B), column c at lds + c CS */
#pragma unroll
	for (int it = 0; it < P; it++) {
		const int r = threadIdx.x / CW + 64 * it, c = threadIdx.x % CW;
		lds[c * CS + sg_strip_row<CW>(r, c)] = base[(size_t)r * S + c];
	}
	__syncthreads();
	float2 v[P];
#pragma unroll
	for (int j = 0; j < P; j++)
		v[j] = col[64 * j + (lane ^ sw)];
	const int km = lane >> 1, hm = lane & 1;
	const int kx = (x0 + wave) & (H - 1);
	/* the reference column's loads (specp: lane order) issued now, in flight during the forward transform */
	float2 r[P];
	if (kx) {
		const float2 *sp = specp + (size_t)kx * S;
#pragma unroll
		for (int k = 0; k < P; k++)
			r[k] = sp[64 * k + lane];
	}
	/* ---- forward ---- */
	sg_fft2048_wave<false>(v, col, tw, lane);
	/* ---- cross power at ky = km + 32 k + 1024 hm ---- */
	/* A packed column 0's wave keeps its LDS column for Z(-ky) and reads its reference column
	 * from spec by ky. */
	if (kx) {
#pragma unroll
		for (int k = 0; k < P; k++)
			v[k] = sg_rconjf(r[k], v[k]);
	} else {	/* packed column: Z = F0 + i FN, the reference likewise; needs Z(-ky) */
		wsync();
#pragma unroll
		for (int k = 0; k < P; k++)
			col[km + 32 * k + 1024 * hm] = v[k];
		wsync();
#pragma unroll
		for (int k = 0; k < P; k++) {
			const int ky = km + 32 * k + 1024 * hm, m = (S - ky) & (S - 1);
			const float2 zk = v[k], zm = col[m], r1 = spec[(size_t)ky * S], r2 = spec[(size_t)m * S];
			const float2 f0 = make_float2(0.5f * (zk.x + zm.x), 0.5f * (zk.y - zm.y));
			const float2 fn = make_float2(0.5f * (zk.y + zm.y), -0.5f * (zk.x - zm.x));
			const float2 r0 = make_float2(0.5f * (r1.x + r2.x), 0.5f * (r1.y - r2.y));
			const float2 rn = make_float2(0.5f * (r1.y + r2.y), -0.5f * (r1.x - r2.x));
			const float2 p0 = sg_rconj(r0, f0), pn = sg_rconj(rn, fn);
			v[k] = make_float2(p0.x - pn.y, p0.y + pn.x);
		}
	}
	/* ---- inverse (unnormalised, FFTW_BACKWARD) ---- */
	{
		const float sg1 = hm ? -1.0f : 1.0f;
		const sg_v2f s2 = sg_v2f{sg1, sg1};
#pragma unroll
		for (int k = 0; k < P; k++)
			v[k] = sg_pm_add(v[k], sg_pair_swap(v[k]), s2);
	}
	if (hm) {
#pragma unroll
		for (int k = 1; k < P; k++) {
			const float2 t = tw[S + 32 * k];
			v[k] = sg_cmulk(v[k], sg_v2f{t.x, t.y});
		}
	}
	sg_dft32_lane<true>(v);
	wsync();
#pragma unroll
	for (int i = 0; i < P; i++)
		col[km * TR + 2 * i + hm] = v[i];
	wsync();
#pragma unroll
	for (int k1 = 0; k1 < P; k1++)
		v[k1] = col[k1 * TR + lane];
	sg_twiddle_rows(v, tw + S, lane);
	sg_dft32_lane<true>(v);
	wsync();
#pragma unroll
	for (int j = 0; j < P; j++)
		col[64 * j + (lane ^ sw)] = v[j];
	__syncthreads();
	{	/* every LDS read issued before the stores (one LDS latency, not eight) */
		float2 o[P];
#pragma unroll
		for (int it = 0; it < P; it++) {
			const int r = threadIdx.x / CW + 64 * it, c = threadIdx.x % CW;
			o[it] = lds[c * CS + sg_strip_row<CW>(r, c)];
		}
#pragma unroll
		for (int it = 0; it < P; it++) {
			const int r = threadIdx.x / CW + 64 * it, c = threadIdx.x % CW;
			base[(size_t)r * S + c] = o[it];
		}
	}
}

/* Wave-level fp32 forward row pass at S = 2048: one wave per row, `rpw` rows per wave (4 rows
 * per workgroup at a time, no block barrier; the wave's next row is fetched while this one is
 * transformed: one row at a time left every wave waiting out the full load latency, 2 waves per
 * SIMD being all the LDS allows), the row of a + i b through sg_fft2048_wave, then staged in
 * natural order in the wave's LDS for the separation into the half spectra A, B
 * (k_reg_rows_fwd_half's arithmetic); the frames' energies summed per wave */
/* QF (SG_REG_QFOLD, A/B): QualityEstimate's SubSample (quality.c:223-234) folded in.  A wave then
 * takes rpw consecutive rows from a multiple of 3 (rpw a multiple of 3), so each 3 x 3 block's three
 * rows pass through one wave: before a row's transform its samples (a | b << 16) go through the
 * wave's LDS, each lane adds the row's three-sample sums of outputs lane + 64 m (m < 11, xs = 682)
 * to registers, and the third row of a block writes the 9-sample means to qbuf (frame q = qbase +
 * 2 pair (+1 for b)) and keeps the middle rows' maximum for qmax (k_quality_sub's arithmetic). */
template <bool QF>
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(SG_WCOL_WPE)))
k_reg_rows_fwd_half_w(SgSel sel, const int *__restrict__ fa, const int *__restrict__ fb,
		const float2 *__restrict__ tw, float2 *__restrict__ work, unsigned long long *__restrict__ energy, int rpw,
		uint16_t *__restrict__ qbuf, unsigned int *__restrict__ qmax, int qbase) {
	constexpr int S = 2048, H = 1024, P = 32;
	constexpr int XS = (S - 1) / 3, YS = (S - 1) / 3, QM = (XS + 63) / 64;
	extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
	const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
	const int row0 = QF ? (blockIdx.x * 4 + wave) * rpw : blockIdx.x * 4 * rpw + wave, pair = blockIdx.y;
	if (QF && row0 >= S)
		return;
	float2 *col = (float2 *)smem + wave * SG_WCOL_CS;
	const size_t plane = (size_t)S * S;
	const uint16_t *pa = sel.frame(fa[pair]);
	const int b = fb[pair];
	const uint16_t *pb = b >= 0 ? sel.frame(b) : nullptr;
	const size_t rp = (size_t)sel.rp;
	uint16_t ua[P], ub[P];
	auto fetch = [&](int row) {
#pragma unroll
		for (int j = 0; j < P; j++)
			ua[j] = pa[(size_t)row * rp + 64 * j + lane];
		if (pb) {
#pragma unroll
			for (int j = 0; j < P; j++)
				ub[j] = pb[(size_t)row * rp + 64 * j + lane];
		}
	};
	fetch(row0);
	unsigned long long ea = 0, eb = 0;
	const int km = lane >> 1, hm = lane & 1;
	uint32_t qa[QM], qb[QM], mxa = 0, mxb = 0;
	if constexpr (QF) {
#pragma unroll
		for (int m = 0; m < QM; m++)
			qa[m] = qb[m] = 0;
	}
	for (int rr = 0; rr < rpw; rr++) {
		const int row = QF ? row0 + rr : row0 + 4 * rr;
		if (QF && row >= S)
			break;
		if constexpr (QF) {	/* the row's samples through LDS, its three-sample sums added */
			uint32_t *cu = (uint32_t *)col;
			if (row < 3 * YS) {
#pragma unroll
				for (int j = 0; j < P; j++)
					cu[64 * j + lane] = (uint32_t)ua[j] | ((uint32_t)(pb ? ub[j] : 0) << 16);
				__builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
#pragma unroll
				for (int m = 0; m < QM; m++) {
					const int i = 64 * m + lane;
					if (i < XS) {
						const uint32_t d0 = cu[3 * i], d1 = cu[3 * i + 1], d2 = cu[3 * i + 2];
						qa[m] += (d0 & 0xFFFFu) + (d1 & 0xFFFFu) + (d2 & 0xFFFFu);
						qb[m] += (d0 >> 16) + (d1 >> 16) + (d2 >> 16);
					}
				}
				__builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");	/* the transform reuses col */
			}
		}
		float2 v[P];
#pragma unroll
		for (int j = 0; j < P; j++) {
			const uint32_t u = ua[j];
			ea += (unsigned long long)(u * u);
			v[j] = make_float2((float)u, 0.0f);
		}
		if (pb) {
#pragma unroll
			for (int j = 0; j < P; j++) {
				const uint32_t u = ub[j];
				eb += (unsigned long long)(u * u);
				v[j].y = (float)u;
			}
		}
		if (QF ? (rr + 1 < rpw && row + 1 < S) : rr + 1 < rpw)
			fetch(QF ? row + 1 : row + 4);
		if constexpr (QF) {	/* a block's third row: the 9-sample means (SubSample, :223-234) */
			if (row % 3 == 2 && row < 3 * YS) {
				const int t = row / 3;
				const bool middle = t >= 1 && t <= YS - 2;
				uint16_t *da = qbuf + (size_t)(qbase + 2 * pair) * XS * YS + (size_t)t * XS;
#pragma unroll
				for (int m = 0; m < QM; m++) {
					const int i = 64 * m + lane;
					const uint32_t va = qa[m] / 9u, vb = qb[m] / 9u;
					if (i < XS) {
						da[i] = (uint16_t)va;
						if (middle && va > 0 && va < 65530 && va > mxa)
							mxa = va;
						if (pb) {
							da[(size_t)XS * YS + i] = (uint16_t)vb;
							if (middle && vb > 0 && vb < 65530 && vb > mxb)
								mxb = vb;
						}
					}
					qa[m] = qb[m] = 0;
				}
			}
		}
		sg_fft2048_wave<false>(v, col, tw, lane);
		__builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
		/* natural order, the upper half 8 entries up: lanes km and km + 8 (hm = 0 / 1) of a
		 * 16-lane store group on different banks */
#pragma unroll
		for (int k = 0; k < P; k++)
			col[km + 32 * k + (1024 + 8) * hm] = v[k];
		__builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
		float2 *out = work + (size_t)pair * plane + (size_t)row * S;
#pragma unroll 4
		for (int q = 0; q < H / 64; q++) {
			const int kx = 64 * q + lane;
			const float2 zk = col[kx], zm = col[(kx ? S - kx : H) + 8];
			float2 A, B;
			if (kx == 0) {
				A = make_float2(zk.x, zm.x);	/* A(0) + i A(S/2) */
				B = make_float2(zk.y, zm.y);
			} else {
				A = make_float2(0.5f * (zk.x + zm.x), 0.5f * (zk.y - zm.y));
				B = make_float2(0.5f * (zk.y + zm.y), -0.5f * (zk.x - zm.x));
			}
			out[kx] = A;
			out[H + kx] = B;
		}
		__builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");	/* the next row's transposes reuse col */
	}
	for (int o = 32; o > 0; o >>= 1) {
		ea += __shfl_xor(ea, o, 64);
		eb += __shfl_xor(eb, o, 64);
	}
	if (lane == 0) {
		atomicAdd(energy + fa[pair], ea);
		if (b >= 0)
			atomicAdd(energy + b, eb);
	}
	if constexpr (QF) {
		for (int o = 32; o > 0; o >>= 1) {
			const uint32_t ta = (uint32_t)__shfl_xor((int)mxa, o, 64), tb = (uint32_t)__shfl_xor((int)mxb, o, 64);
			mxa = ta > mxa ? ta : mxa;
			mxb = tb > mxb ? tb : mxb;
		}
		if (lane == 0 && mxa)
			atomicMax(qmax + qbase + 2 * pair, mxa);
		if (lane == 0 && mxb)
			atomicMax(qmax + qbase + 2 * pair + 1, mxb);
	}
}

/* Wave-level fp32 inverse row pass + arg-max at S = 2048: one wave per row; the packed
 * spectrum Qa + i Qb rebuilt per element as k_reg_rows_inv_half_argmax does, the inverse
 * transform by sg_fft2048_wave<true> (its permuted output order only changes which index a
 * value carries), the row's top-2 reduced in the wave */
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(SG_WCOL_WPE)))
k_reg_rows_inv_half_w(const float2 *__restrict__ work, const float2 *__restrict__ tw, SgBest *__restrict__ best) {
	constexpr int S = 2048, H = 1024, P = 32;
	extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
	const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
	const int row = blockIdx.x * 4 + wave, pair = blockIdx.y;
	float2 *col = (float2 *)smem + wave * SG_WCOL_CS;
	const float2 *in = work + (size_t)pair * S * S + (size_t)row * S;
	float2 v[P];
	/* every load unconditional (all 64 in flight; the packed-pair lane's branch had split them
	 * into dependent groups), the packing and conjugation applied after */
	float2 ra[P], rb[P];
#pragma unroll
	for (int j = 0; j < P; j++) {
		const int i = 64 * j + lane;
		const int src = (i & (H - 1)) == 0 ? 0 : (i < H ? i : S - i);
		ra[j] = in[src];
		rb[j] = in[H + src];
	}
#pragma unroll
	for (int j = 0; j < P; j++) {
		const int i = 64 * j + lane;
		float2 qa = ra[j], qb = rb[j];
		if ((i & (H - 1)) == 0) {	/* kx = 0 or S/2: the packed real pair */
			qa = make_float2(i ? qa.y : qa.x, 0.0f);
			qb = make_float2(i ? qb.y : qb.x, 0.0f);
		} else if (i >= H) {
			qa.y = -qa.y;
			qb.y = -qb.y;
		}
		v[j] = make_float2(qa.x - qb.y, qa.y + qb.x);
	}
	sg_fft2048_wave<true>(v, col, tw, lane);
	const int km = lane >> 1, hm = lane & 1;
	SgTop2T<float> ta, tb;
	sg_top2t_init(ta);
	sg_top2t_init(tb);
#pragma unroll
	for (int k = 0; k < P; k++) {
		const int idx = row * S + km + 32 * k + 1024 * hm;
		sg_top2t_add_inc(ta, v[k].x, idx);	/* idx grows with k */
		sg_top2t_add_inc(tb, v[k].y, idx);
	}
	sg_top2t_wave(ta);
	sg_top2t_wave(tb);
	const SgTop2 wa = sg_top2t_wide(ta), wb = sg_top2t_wide(tb);
	if (lane == 0) {
		best[(size_t)pair * S + row].a = wa;
		best[(size_t)pair * S + row].b = wb;
	}
}

/* per-pair result of a registration batch (frame a = the real part, frame b = the imaginary) */
struct SgRegOut {
	int sx[2], sy[2];	/* the shifts (:344-351) */
	int idx[2];		/* arg-max (row-major) */
	int amb[2];		/* near tie: the runner-up lies within `tol` of the maximum */
	double v[2], v2[2], thr[2];	/* maximum, runner-up, max - tol */
};

/* tolerance of a correlation value: 2^tol_exp S^2 ||ref|| ||img|| (the unnormalised inverse
 * scales the exact correlation sum_n ref(n+k) img(n) by S^2, and by Cauchy-Schwarz no entry
 * exceeds S^2 ||ref|| ||img||).  fp64 passes: 2^-32, many orders of magnitude above their
 * rounding; fp32 passes: 2^-15 = 3.1e-5, against a measured worst error of 2.8e-7 of that scale
 * at S = 2048 (scipy's complex64 FFT, the synthetic pair) and a log2(S^2) eps32 bound of 1.3e-6
 * per transform.  A maximum that beats every other entry by more than tol is the exact
 * maximum. */
__device__ __forceinline__ double sg_reg_tol(int S, unsigned long long eref, unsigned long long eimg, int tol_exp) {
	return ldexp((double)S * (double)S * sqrt((double)eref) * sqrt((double)eimg), tol_exp);
}

/* per pair: reduce the row / strip partials in order, convert to (shiftx, shifty) (:344-351),
 * flag near ties against the frames' energies */
__global__ void __launch_bounds__(256)
k_reg_final(const SgBest *__restrict__ best, int S, int count, const int *__restrict__ fa,
		const int *__restrict__ fb, int ref, const unsigned long long *__restrict__ energy, int tol_exp,
		SgRegOut *__restrict__ out) {
	__shared__ SgBest red[4];
	const int pair = blockIdx.x;
	SgTop2 ta, tb;
	sg_top2_init(ta);
	sg_top2_init(tb);
	for (int r = threadIdx.x; r < count; r += blockDim.x) {
		const SgBest b = best[(size_t)pair * count + r];
		sg_top2_merge(ta, b.a.v, b.a.v2, b.a.i);
		sg_top2_merge(tb, b.b.v, b.b.v2, b.b.i);
	}
	sg_best_block(ta, tb, red);
	if (threadIdx.x == 0) {
		SgRegOut o;
		const SgTop2 t[2] = {ta, tb};
		const int fr[2] = {fa[pair], fb[pair]};
		for (int k = 0; k < 2; k++) {
			int sy = t[k].i / S, sx = t[k].i % S;
			if (sy > S / 2)
				sy -= S;
			if (sx > S / 2)
				sx -= S;
			o.sx[k] = sx;
			o.sy[k] = sy;
			o.idx[k] = t[k].i;
			o.v[k] = t[k].v;
			o.v2[k] = t[k].v2;
			const double tol = fr[k] >= 0 ? sg_reg_tol(S, energy[ref], energy[fr[k]], tol_exp) : 0.0;
			o.thr[k] = t[k].v - tol;
			o.amb[k] = fr[k] >= 0 && !(t[k].v - t[k].v2 > tol);
		}
		out[pair] = o;
	}
}

/* CAND: instead of the arg-max, append every index whose correlation reaches the pair's
 * threshold (SgRegOut::thr, near ties only) to the candidate list of its frame */
template <class C, bool CAND>
__global__ void __launch_bounds__(512)
k_reg_rows_inv_half_argmax(const C *__restrict__ work, int S, const C *__restrict__ tw,
		SgBest *__restrict__ best, const SgRegOut *__restrict__ res, SgCand *__restrict__ cand) {
	extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
	C *buf = (C *)smem;
	__shared__ SgBest red[8];
	const int row = blockIdx.x, pair = blockIdx.y, H = S >> 1;
	const C *in = work + (size_t)pair * S * S + (size_t)row * S;
	typedef typename SgReal<C>::T T;
	SgTop2T<T> ta, tb;
	sg_top2t_init(ta);
	sg_top2t_init(tb);
	double thr[2] = {INFINITY, INFINITY};
	if (CAND) {
		const SgRegOut r = res[pair];
		if (!r.amb[0] && !r.amb[1])
			return;
		thr[0] = r.amb[0] ? r.thr[0] : INFINITY;
		thr[1] = r.amb[1] ? r.thr[1] : INFINITY;
	}
	sg_fft_io(buf, S, 1, S, tw, true,
			[&](int, int i) {
				C qa, qb;
				if ((i & (H - 1)) == 0) {	/* kx = 0 or S/2: the packed real pair */
					const C a = in[0], b = in[H];
					qa = sg_mk<C>(i ? a.y : a.x, (T)0);
					qb = sg_mk<C>(i ? b.y : b.x, (T)0);
				} else if (i < H) {
					qa = in[i];
					qb = in[H + i];
				} else {
					const C a = in[S - i], b = in[H + S - i];
					qa = sg_mk<C>(a.x, -a.y);
					qb = sg_mk<C>(b.x, -b.y);
				}
				return sg_mk<C>(qa.x - qb.y, qa.y + qb.x);
			},
			[&](int, int j, C c) {
				const int idx = row * S + j;
				if (CAND) {
					sg_cand_push(cand + 2 * pair, c.x, thr[0], idx);
					sg_cand_push(cand + 2 * pair + 1, c.y, thr[1], idx);
					return;
				}
				sg_top2t_add(ta, c.x, idx);
				sg_top2t_add(tb, c.y, idx);
			});
	if (CAND)
		return;
	SgTop2 wa = sg_top2t_wide(ta), wb = sg_top2t_wide(tb);
	sg_best_block(wa, wb, red);
	if (threadIdx.x == 0) {
		best[(size_t)pair * S + row].a = wa;
		best[(size_t)pair * S + row].b = wb;
	}
}

/* ---------------------------------------------------------------------------------------
 * QualityEstimate (src/algos/quality.c).  Only subsample 3 contributes to the result:
 * dval += q * ((QSUBSAMPLE_MIN * QSUBSAMPLE_MIN) / (subsample * subsample)) uses integer
 * division (:211), so the factor is 1 for subsample 3 and 0 for 4 and 5.
 * ------------------------------------------------------------------------------------- */
#define SG_Q_THRESHOLD (40 << 8)
#define SG_QROWS 4	/* subsampled rows per k_quality_sub workgroup */

/* SubSample (:223-234) of one 3x3 sample row, plus the running max of the middle rows
 * (the maxp[] loop :119-133 reduces to max over 0 < v < 65530) */
__global__ void __launch_bounds__(1024)
k_quality_sub(SgSel sel, int al, const int *__restrict__ qframes, int S, int xs, int ys,
		uint16_t *__restrict__ qbuf, unsigned int *__restrict__ qmax) {
	/* SG_QROWS output rows per workgroup; a thread forms two adjacent outputs from three
	 * 12-byte (6-pixel, dword-aligned) loads, one per input row */
	const int q = blockIdx.y;
	const uint16_t *frame = sel.frame(qframes[q]);
	unsigned int m = 0;
	const int j0 = blockIdx.x * SG_QROWS;
	for (int k = threadIdx.x; 2 * k < xs; k += blockDim.x) {
		/* the 3 x SG_QROWS input rows of this pair: every load issued before any is used */
		uint32_t d[SG_QROWS][3][3];
#pragma unroll
		for (int jj = 0; jj < SG_QROWS; jj++) {
			const int j = j0 + jj < ys ? j0 + jj : ys - 1;
#pragma unroll
			for (int y = 0; y < 3; y++) {
				const uint16_t *q16 = frame + (size_t)(3 * j + y) * sel.rp + 6 * k;
				if (al) {	/* even side, pitches and base: the 12 bytes are dword aligned */
					const uint32_t *p = (const uint32_t *)q16;
					d[jj][y][0] = p[0];
					d[jj][y][1] = p[1];
					d[jj][y][2] = p[2];
				} else {
					d[jj][y][0] = (uint32_t)q16[0] | ((uint32_t)q16[1] << 16);
					d[jj][y][1] = (uint32_t)q16[2] | ((uint32_t)q16[3] << 16);
					d[jj][y][2] = (uint32_t)q16[4] | ((uint32_t)q16[5] << 16);
				}
			}
		}
#pragma unroll
		for (int jj = 0; jj < SG_QROWS; jj++) {
			const int j = j0 + jj;
			if (j >= ys)
				break;
			const bool middle = (j >= 1 && j <= ys - 2);
			uint16_t *dst = qbuf + (size_t)q * xs * ys + (size_t)j * xs;
			int va = 0, vb = 0;
#pragma unroll
			for (int y = 0; y < 3; y++) {
				const uint32_t d0 = d[jj][y][0], d1 = d[jj][y][1], d2 = d[jj][y][2];
				va += (int)(d0 & 0xFFFFu) + (int)(d0 >> 16) + (int)(d1 & 0xFFFFu);
				vb += (int)(d1 >> 16) + (int)(d2 & 0xFFFFu) + (int)(d2 >> 16);
			}
			va /= 9;
			vb /= 9;
			dst[2 * k] = (uint16_t)va;
			if (middle && va > 0 && va < 65530 && (unsigned)va > m)
				m = (unsigned)va;
			if (2 * k + 1 < xs) {
				dst[2 * k + 1] = (uint16_t)vb;
				if (middle && vb > 0 && vb < 65530 && (unsigned)vb > m)
					m = (unsigned)vb;
			}
		}
	}
	for (int o = 32; o > 0; o >>= 1) {
		const unsigned int t = (unsigned int)__shfl_down((int)m, o, 64);
		m = t > m ? t : m;
	}
	if ((threadIdx.x & 63) == 0 && m)
		atomicMax(qmax + q, m);
}

/* _smooth_image_16 (:324-349) + Gradient (:236-321): threshold map dilated 3x3 inside the
 * 10 % margins, gradient energy over mapped pixels; exact integer sums.  Streamed down a band:
 * one wave per (60-column band, SG_QGS_ROWS output rows, frame) of the margins' interior, lane l
 * at column x0 - 2 + l.  Each input row is loaded and stretched once (:139-148: v * (60000 / max),
 * truncated, clamped at 65535; SG_QGS_PF rows in flight), its horizontal 3-sum formed with two
 * lane shuffles, and rolling three-row windows give the smoothed row, the thresholded map and the
 * gradient of output row y as rows y + 2 arrive.  Only the interior's neighbourhood is read, and
 * no LDS or barrier: 190 us per configs[1] step against 290 for the tiled kernel it replaced
 * (64 x 16 output tiles through LDS, 61 k workgroups; removed, commit 9b01e1f last contained it),
 * registration 3.20 -> 3.10 ms (profiles/r05x_*). */
#define SG_QGS_ROWS 64
#define SG_QGS_PF 8
__global__ void __launch_bounds__(64)
k_quality_grad_s(const uint16_t *__restrict__ qbuf, int xs, int ys, const unsigned int *__restrict__ qmax,
		unsigned long long *__restrict__ acc) {
	const int q = blockIdx.z, lane = threadIdx.x;
	const uint16_t *b = qbuf + (size_t)q * xs * ys;
	const unsigned int mx = qmax[q];
	const bool stretch = mx > 0;
	const double mult = stretch ? (double)60000 / (double)mx : 1.0;
	const int yb = (int)((double)ys * 0.1) + 1;
	const int xb = (int)((double)xs * 0.1) + 1;
	const int x0 = xb + 60 * blockIdx.x, c = x0 - 2 + lane;
	const int y0 = yb + SG_QGS_ROWS * blockIdx.y;
	const int y1 = min(y0 + SG_QGS_ROWS, ys - yb);	/* output rows [y0, y1) */
	const bool in_x = c >= xb && c < xs - xb;	/* the map's and the output's column range */
	const bool out_lane = lane >= 2 && lane < 62 && in_x;
	const bool col_ok = c >= 0 && c < xs, sm_x = c >= 1 && c <= xs - 2;
	unsigned long long val = 0;
	unsigned int pix = 0, cnt = 0;
	/* rolling state: horizontal sums of the last three stretched rows, the last two smoothed
	 * rows (value, right neighbour's) and the last two rows' horizontally OR-ed map bits */
	unsigned int h0 = 0, h1 = 0;
	int sm_prev = 0, smr_prev = 0;
	bool th_prev2 = false, th_prev = false;
	const int ya = y0 - 2, yz = y1 + 1;	/* input rows [ya, yz] */
	for (int g = ya; g <= yz; g += SG_QGS_PF) {
		unsigned int raw[SG_QGS_PF];
#pragma unroll
		for (int k = 0; k < SG_QGS_PF; k++) {
			const int yi = g + k;
			raw[k] = (col_ok && yi >= 0 && yi < ys && yi <= yz) ? (unsigned int)b[(size_t)yi * xs + c] : 0u;
		}
#pragma unroll
		for (int k = 0; k < SG_QGS_PF; k++) {
			const int yi = g + k;
			if (yi > yz)
				break;
			unsigned int st = raw[k];
			if (stretch && col_ok && yi >= 0 && yi < ys) {
				st = (unsigned int)((double)st * mult);
				if (st > 65535u)
					st = 65535u;
			}
			const unsigned int h = st + (unsigned int)__shfl_up((int)st, 1, 64) + (unsigned int)__shfl_down((int)st, 1, 64);
			if (yi >= ya + 2) {
				/* smoothed row qy = yi - 1 from the horizontal sums of rows yi - 2 .. yi */
				const int qy = yi - 1;
				const int sm = (sm_x && qy >= 1 && qy <= ys - 2) ? (int)((h0 + h1 + h) / 9) : 0;
				const bool thr = sm >= SG_Q_THRESHOLD && in_x && qy >= yb && qy < ys - yb;
				/* both shuffles by every lane (a short-circuit || would run them under a partial
				 * exec mask) */
				const int thn = (int)thr, thl = __shfl_up(thn, 1, 64), thr1 = __shfl_down(thn, 1, 64);
				const bool th = (thn | thl | thr1) != 0;
				const int smr = __shfl_down(sm, 1, 64);
				/* output row yo = qy - 1: its row (sm_prev), the row below (sm), the map rows
				 * yo - 1 .. yo + 1 */
				const int yo = qy - 1;
				if (yo >= y0 && out_lane) {
					if (sm_prev >= SG_Q_THRESHOLD)
						cnt++;
					if (th_prev2 || th_prev || th) {
						const long long d1 = sm_prev - smr_prev;
						const long long d2 = sm_prev - sm;
						val += (unsigned long long)(d1 * d1 + d2 * d2);
						pix++;
					}
				}
				sm_prev = sm;
				smr_prev = smr;
				th_prev2 = th_prev;
				th_prev = th;
			}
			h0 = h1;
			h1 = h;
		}
	}
	unsigned long long p = pix, n = cnt;
	for (int o = 32; o > 0; o >>= 1) {
		val += __shfl_down(val, o, 64);
		p += __shfl_down(p, o, 64);
		n += __shfl_down(n, o, 64);
	}
	if (lane == 0) {
		if (val)
			atomicAdd(acc + q * 3, val);
		if (p)
			atomicAdd(acc + q * 3 + 1, p);
		if (n)
			atomicAdd(acc + q * 3 + 2, n);
	}
}

/* ---------------------------------------------------------------------------------------
 * Any selection side (FFTW plans every S, registration.c:251-257): mixed-radix Stockham
 * passes (radix 8, 4, 2, 3, 5, 7) in LDS, one line per workgroup, ping-pong between two LDS
 * buffers; a side with a prime factor above 7 goes through Bluestein's chirp-z transform
 * (X_k = c_k sum_j (x_j c_j) conj(c_{k-j}), c_j = exp(-i pi j^2 / n), as an M-point power-of-two
 * convolution, M >= 2n - 1).  Columns are transformed as rows of the transposed plane:
 *   rows(u16 -> spectrum) -> transpose -> rows -> cross power -> inverse rows -> transpose ->
 *   inverse rows + top-2 arg-max.
 * Same unnormalised FFTW_FORWARD / FFTW_BACKWARD convention and pair packing (a + i b) as the
 * power-of-two passes; the cross power works on the transposed spectra directly (the mirror of
 * (r, c) is ((S - r) % S, (S - c) % S) in either layout).
 * ------------------------------------------------------------------------------------- */
/* cos / sin of 2 pi m / R, m < R (R = 3, 5, 7) */
template <int R>
__device__ __forceinline__ void sg_unit(int m, double &c, double &s) {
	if (m == 0) {
		c = 1.0;
		s = 0.0;
		return;
	}
	const int mm = m <= R / 2 ? m : R - m;
	const double sg = m <= R / 2 ? 1.0 : -1.0;
	if constexpr (R == 3) {
		c = -0.5;
		s = 0.86602540378443864676;
	} else if constexpr (R == 5) {
		c = mm == 1 ? 0.30901699437494742410 : -0.80901699437494742410;
		s = mm == 1 ? 0.95105651629515357212 : 0.58778525229247312917;
	} else {
		c = mm == 1 ? 0.62348980185873353053 : (mm == 2 ? -0.22252093395631440429 : -0.90096886790241912624);
		s = mm == 1 ? 0.78183148246802980871 : (mm == 2 ? 0.97492791218182360702 : 0.43388373911755812048);
	}
	s *= sg;
}

/* in-register DFT of an odd prime R: y_k = sum_j v_j w^{jk}, w = exp(-+2 pi i / R), from the
 * symmetric sums t_j = v_j + v_{R-j} and differences u_j = v_j - v_{R-j} (j <= R/2): y_k and
 * y_{R-k} share a = v_0 + sum_j t_j cos(2 pi jk / R) and b = sum_j u_j sin(2 pi jk / R),
 * y_k = a -+ i b, y_{R-k} = a +- i b (half the multiplies of the direct sum and ~half its live
 * registers: the radix-7 pass spilled at 128 VGPRs with the direct form).  Its rounding is far
 * below the fp64 tie tolerance (sg_reg_tol). */
template <int R>
__device__ __forceinline__ void sg_dft_odd(sg_c64 (&v)[R], bool inv) {
	constexpr int H = R / 2;
	sg_c64 t[H + 1], u[H + 1];
	double y0x = v[0].x, y0y = v[0].y;
#pragma unroll
	for (int j = 1; j <= H; j++) {
		t[j] = make_double2(v[j].x + v[R - j].x, v[j].y + v[R - j].y);
		u[j] = make_double2(v[j].x - v[R - j].x, v[j].y - v[R - j].y);
		y0x += t[j].x;
		y0y += t[j].y;
	}
#pragma unroll
	for (int k = 1; k <= H; k++) {
		double ax = v[0].x, ay = v[0].y, bx = 0.0, by = 0.0;
#pragma unroll
		for (int j = 1; j <= H; j++) {
			double c, sn;
			sg_unit<R>((j * k) % R, c, sn);
			ax += t[j].x * c;
			ay += t[j].y * c;
			bx += u[j].x * sn;
			by += u[j].y * sn;
		}
		/* forward: y_k = a - i b = (ax + by, ay - bx); inverse: a + i b */
		if (!inv) {
			v[k] = make_double2(ax + by, ay - bx);
			v[R - k] = make_double2(ax - by, ay + bx);
		} else {
			v[k] = make_double2(ax - by, ay + bx);
			v[R - k] = make_double2(ax + by, ay - bx);
		}
	}
	v[0] = make_double2(y0x, y0y);
}

/* Mixed-radix Stockham passes on one line, in place in ONE LDS buffer (72 KB at S = 4000, so
 * two workgroups share a CU; the round-3 ping-pong between two buffers held one workgroup of 4
 * waves per CU).  Work item j of a radix-R pass (j < n / R, k = j mod Ns) reads elements
 * j + r n / R, twiddles them by w^(r k n / (Ns R)), and writes (j - k) R + k + r Ns: every item's
 * inputs are loaded into registers before the barrier and stored after it.  The first pass reads
 * the line straight from memory (ld(i)), the last pass hands its outputs to st(i, v): two LDS
 * round trips fewer.  Items per thread: blockDim >= n / 8, and >= n / 7 when 7 divides n (host-
 * sized), so a radix-R pass has at most 4 (R = 2), 3 (3), 2 (4, 5) or 1 (7, 8) items per thread
 * (two radix-7 items per thread spilled at the 128 VGPRs of two workgroups per CU). */
template <int R> struct SgGenItems { static constexpr int v = R == 2 ? 4 : (R == 3 ? 3 : (R == 8 || R == 7 ? 1 : 2)); };

template <int R, bool IN_MEM, bool OUT_MEM, class LD, class ST>
__device__ __forceinline__ void sg_gen_pass_ip(sg_c64 *buf, int n, int Ns, const sg_c64 *__restrict__ tw, bool inv,
		LD &ld, ST &st, int tid, int nt) {
	constexpr int MAXI = SgGenItems<R>::v;
	const int per = n / R, tstep = n / (Ns * R);
	sg_c64 v[MAXI][R];
#pragma unroll
	for (int it = 0; it < MAXI; it++) {
		const int j = tid + it * nt;
		if (j < per) {
			const int k = j % Ns;
#pragma unroll
			for (int r = 0; r < R; r++)
				v[it][r] = IN_MEM ? ld(j + r * per) : buf[sg_pad(j + r * per)];
			if (Ns > 1) {
#pragma unroll
				for (int r = 1; r < R; r++)
					v[it][r] = sg_cmul(v[it][r], sg_twiddle(tw, n, r * k * tstep, inv));
			}
		}
	}
	if (!IN_MEM && !OUT_MEM)
		__syncthreads();	/* in place: every input read before any output lands */
#pragma unroll
	for (int it = 0; it < MAXI; it++) {
		const int j = tid + it * nt;
		if (j < per) {
			const int k = j % Ns;
			if constexpr (R == 2 || R == 4 || R == 8)
				sg_dft_small<R, R>(v[it], inv);
			else
				sg_dft_odd<R>(v[it], inv);
			const int base = (j - k) * R + k;
#pragma unroll
			for (int r = 0; r < R; r++) {
				if (OUT_MEM)
					st(base + r * Ns, v[it][r]);
				else
					buf[sg_pad(base + r * Ns)] = v[it][r];
			}
		}
	}
	if (!OUT_MEM)
		__syncthreads();
}

template <bool IN_MEM, bool OUT_MEM, class LD, class ST>
__device__ __forceinline__ void sg_gen_pass_r(int R, sg_c64 *buf, int n, int Ns, const sg_c64 *__restrict__ tw, bool inv,
		LD &ld, ST &st, int tid, int nt) {
	switch (R) {
	case 8: sg_gen_pass_ip<8, IN_MEM, OUT_MEM>(buf, n, Ns, tw, inv, ld, st, tid, nt); break;
	case 4: sg_gen_pass_ip<4, IN_MEM, OUT_MEM>(buf, n, Ns, tw, inv, ld, st, tid, nt); break;
	case 2: sg_gen_pass_ip<2, IN_MEM, OUT_MEM>(buf, n, Ns, tw, inv, ld, st, tid, nt); break;
	case 3: sg_gen_pass_ip<3, IN_MEM, OUT_MEM>(buf, n, Ns, tw, inv, ld, st, tid, nt); break;
	case 5: sg_gen_pass_ip<5, IN_MEM, OUT_MEM>(buf, n, Ns, tw, inv, ld, st, tid, nt); break;
	default: sg_gen_pass_ip<7, IN_MEM, OUT_MEM>(buf, n, Ns, tw, inv, ld, st, tid, nt); break;
	}
}

/* the n-point transform of the line, natural order in and out: FROM_MEM reads it through
 * ld(0..n) (else it is in buf, written and synchronised by the caller), TO_MEM hands the result
 * to st(0..n) (else it is left in buf, synchronised).  Threads tid < nt of the block take part
 * (a block may run one line per part, all parts through the same passes and barriers). */
template <bool FROM_MEM, bool TO_MEM, class LD, class ST>
__device__ __forceinline__ void sg_gen_fft_mixed(sg_c64 *buf, const SgGenPlan &pl, const sg_c64 *__restrict__ tw, bool inv, LD &ld,
		ST &st, int tid, int nt) {
	const int n = pl.n;
	if (pl.npass == 1) {
		if (FROM_MEM || TO_MEM) {
			sg_gen_pass_r<FROM_MEM, TO_MEM>(pl.radix[0], buf, n, 1, tw, inv, ld, st, tid, nt);
		} else {
			sg_gen_pass_r<false, false>(pl.radix[0], buf, n, 1, tw, inv, ld, st, tid, nt);
		}
		return;
	}
	sg_gen_pass_r<FROM_MEM, false>(pl.radix[0], buf, n, 1, tw, inv, ld, st, tid, nt);
	int Ns = pl.radix[0];
	for (int q = 1; q + 1 < pl.npass; q++) {
		sg_gen_pass_r<false, false>(pl.radix[q], buf, n, Ns, tw, inv, ld, st, tid, nt);
		Ns *= pl.radix[q];
	}
	sg_gen_pass_r<false, TO_MEM>(pl.radix[pl.npass - 1], buf, n, Ns, tw, inv, ld, st, tid, nt);
}

/* Bluestein: x (n values at buf[pad(0..n)], written and synchronised by the caller) -> X in
 * place.  The inverse is conj(forward(conj x)).  twm: twiddles of the m-point transforms,
 * chirp: c_j (j < n), bhat: FFT_m of b (b_j = conj c_|j|, wrapped). */
__device__ void sg_gen_fft_bluestein(sg_c64 *buf, const SgGenPlan &pl, const sg_c64 *__restrict__ twm,
		const sg_c64 *__restrict__ chirp, const sg_c64 *__restrict__ bhat, bool inv) {
	const int n = pl.n, m = pl.m;
	for (int j = threadIdx.x; j < m; j += blockDim.x) {
		sg_c64 a = make_double2(0.0, 0.0);
		if (j < n) {
			sg_c64 x = buf[sg_pad(j)];
			if (inv)
				x.y = -x.y;
			a = sg_cmul(x, chirp[j]);
		}
		buf[sg_pad(j)] = a;
	}
	sg_lds_fft(buf, m, 0, 1, m, twm, false);
	for (int j = threadIdx.x; j < m; j += blockDim.x)
		buf[sg_pad(j)] = sg_cmul(buf[sg_pad(j)], bhat[j]);
	sg_lds_fft(buf, m, 0, 1, m, twm, true);
	const double sc = 1.0 / (double)m;	/* exact: m is a power of two */
	for (int j = threadIdx.x; j < n; j += blockDim.x) {
		sg_c64 y = sg_cmul(buf[sg_pad(j)], chirp[j]);
		y.x *= sc;
		y.y *= sc;
		if (inv)
			y.y = -y.y;
		buf[sg_pad(j)] = y;
	}
	__syncthreads();
}

struct SgGenTables {
	const sg_c64 *tw, *twm, *chirp, *bhat;
};

enum { SG_GEN_FWD_U16 = 0, SG_GEN_C2C = 1, SG_GEN_INV_ARGMAX = 2, SG_GEN_INV_CAND = 3 };

/* one row of pair blockIdx.y: mode FWD_U16 (u16 rows of frames fa / fb packed a + i b, forward,
 * energies), C2C (in place, forward or inverse), INV_ARGMAX (inverse, top-2 arg-max over the
 * row), INV_CAND (inverse, candidates of a near tie) */
template <bool BLUE>
__global__ void __launch_bounds__(BLUE ? 1024 : 640) __attribute__((amdgpu_waves_per_eu(BLUE ? 1 : 4)))
k_gen_rows(SgSel sel, const int *__restrict__ fa, const int *__restrict__ fb,
		sg_c64 *__restrict__ data, int S, SgGenPlan pl, SgGenTables tb, int mode, int inverse,
		unsigned long long *__restrict__ energy, SgBest *__restrict__ best, const SgRegOut *__restrict__ res,
		SgCand *__restrict__ cand) {
	extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
	__shared__ SgBest red[16];
	sg_c64 *b0 = (sg_c64 *)smem;
	const int row = blockIdx.x, pair = blockIdx.y;
	sg_c64 *line = data + ((size_t)pair * S + row) * S;
	const bool inv = mode >= SG_GEN_INV_ARGMAX || (mode == SG_GEN_C2C && inverse);
	double thr[2] = {INFINITY, INFINITY};
	if (mode == SG_GEN_INV_CAND) {
		const SgRegOut r = res[pair];
		if (!r.amb[0] && !r.amb[1])
			return;
		thr[0] = r.amb[0] ? r.thr[0] : INFINITY;
		thr[1] = r.amb[1] ? r.thr[1] : INFINITY;
	}
	const uint16_t *pa = nullptr, *pb = nullptr;
	const int b = mode == SG_GEN_FWD_U16 ? fb[pair] : -1;
	if (mode == SG_GEN_FWD_U16) {
		pa = sel.frame(fa[pair]) + (size_t)row * sel.rp;
		pb = b >= 0 ? sel.frame(b) + (size_t)row * sel.rp : nullptr;
	}
	if (mode == SG_GEN_FWD_U16) {	/* the frames' energies (the rows are read again by the transform, from cache) */
		unsigned long long ea = 0, eb = 0;
		for (int i = threadIdx.x; i < S; i += blockDim.x) {
			const unsigned int va = pa[i], vb = pb ? pb[i] : 0u;
			ea += (unsigned long long)(va * va);
			eb += (unsigned long long)(vb * vb);
		}
		sg_energy_add(ea, eb, fa[pair], b, energy);
	}
	SgTop2 ta, tbv;
	sg_top2_init(ta);
	sg_top2_init(tbv);
	/* element i of the input line (FWD_U16: frames a + i b) */
	auto ld = [&](int i) -> sg_c64 {
		if (mode == SG_GEN_FWD_U16)
			return make_double2((double)pa[i], pb ? (double)pb[i] : 0.0);
		return line[i];
	};
	/* element i of the transformed line */
	auto st = [&](int i, sg_c64 c) {
		if (mode <= SG_GEN_C2C) {
			line[i] = c;
		} else if (mode == SG_GEN_INV_CAND) {
			sg_cand_push(cand + 2 * pair, c.x, thr[0], row * S + i);
			sg_cand_push(cand + 2 * pair + 1, c.y, thr[1], row * S + i);
		} else {
			sg_top2_add(ta, c.x, row * S + i);
			sg_top2_add(tbv, c.y, row * S + i);
		}
	};
	if constexpr (BLUE) {
		for (int i = threadIdx.x; i < S; i += blockDim.x)
			b0[sg_pad(i)] = ld(i);
		__syncthreads();
		sg_gen_fft_bluestein(b0, pl, tb.twm, tb.chirp, tb.bhat, inv);
		for (int i = threadIdx.x; i < S; i += blockDim.x)
			st(i, b0[sg_pad(i)]);
	} else {
		sg_gen_fft_mixed<true, true>(b0, pl, tb.tw, inv, ld, st, (int)threadIdx.x, (int)blockDim.x);
	}
	if (mode <= SG_GEN_C2C || mode == SG_GEN_INV_CAND)
		return;
	sg_best_block(ta, tbv, red);
	if (threadIdx.x == 0) {
		best[(size_t)pair * S + row].a = ta;
		best[(size_t)pair * S + row].b = tbv;
	}
}

/* out[pair][x][y] = in[pair][y][x] (32 x 32 tiles in LDS) */
__global__ void __launch_bounds__(256)
k_gen_transpose(const sg_c64 *__restrict__ in, sg_c64 *__restrict__ out, int S) {
	__shared__ sg_c64 tile[32][33];
	const size_t plane = (size_t)S * S;
	const sg_c64 *src = in + (size_t)blockIdx.z * plane;
	sg_c64 *dst = out + (size_t)blockIdx.z * plane;
	const int x0 = blockIdx.x * 32, y0 = blockIdx.y * 32;
	for (int r = threadIdx.y; r < 32; r += 8) {
		const int y = y0 + r, x = x0 + threadIdx.x;
		if (y < S && x < S)
			tile[r][threadIdx.x] = src[(size_t)y * S + x];
	}
	__syncthreads();
	for (int r = threadIdx.y; r < 32; r += 8) {
		const int x = x0 + r, y = y0 + threadIdx.x;
		if (y < S && x < S)
			dst[(size_t)x * S + y] = tile[threadIdx.x][r];
	}
}

/* separate the packed spectra and form the packed cross-power spectrum, in place, for any S
 * (k_reg_xpower with modular mirrors) */
__global__ void __launch_bounds__(256)
k_gen_xpower(sg_c64 *__restrict__ work, const sg_c64 *__restrict__ spec, int S) {
	const size_t plane = (size_t)S * S;
	sg_c64 *Z = work + (size_t)blockIdx.y * plane;
	for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < plane; i += (size_t)gridDim.x * blockDim.x) {
		const int r = (int)(i / S), c = (int)(i - (size_t)r * S);
		const size_t m = (size_t)(r ? S - r : 0) * S + (c ? S - c : 0);
		if (m < i)
			continue;
		const sg_c64 zk = Z[i], zm = Z[m];
		Z[i] = sg_xpower_at(zk, zm, spec[i]);
		if (m != i)
			Z[m] = sg_xpower_at(zm, zk, spec[m]);
	}
}

/* The generic column passes fused (mixed-radix plans): rows kx and (S - kx) mod S of the
 * transposed spectrum planes (spectrum columns) in one workgroup, each half of the block one
 * row through the same passes and barriers.  Forward transform in LDS, the packed cross power
 * (the mirror of (kx, ky) is ((S - kx) mod S, (S - ky) mod S): the other row), inverse
 * transform stored back: 3 plane passes instead of the 7 of rows + k_gen_xpower + rows.  Rows
 * 0 and S/2 are their own mirror (the second half idles through the barriers).  blockDim =
 * 2 x the row kernel's thread count (<= 1024), LDS two padded rows. */
__global__ void __launch_bounds__(1024) __attribute__((amdgpu_waves_per_eu(4)))
k_gen_cols_xpower(sg_c64 *__restrict__ data, const sg_c64 *__restrict__ spec, int S, SgGenPlan pl,
		const sg_c64 *__restrict__ tw) {
	extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
	const int T = (int)blockDim.x >> 1, half = (int)threadIdx.x >= T ? 1 : 0, tid = (int)threadIdx.x - half * T;
	const int kx = blockIdx.x, pair = blockIdx.y, kxm = kx ? S - kx : 0;
	const bool single = kxm == kx, active = !(single && half);
	const int row = half ? kxm : kx;
	sg_c64 *buf = (sg_c64 *)smem + half * SG_PADN(S);
	const sg_c64 *oth = (const sg_c64 *)smem + (single ? 0 : 1 - half) * SG_PADN(S);
	sg_c64 *line = data + ((size_t)pair * S + row) * S;
	auto ld = [&](int i) -> sg_c64 { return active ? line[i] : make_double2(0.0, 0.0); };
	auto st = [&](int i, sg_c64 v) {
		if (active)
			line[i] = v;
	};
	sg_gen_fft_mixed<true, false>(buf, pl, tw, false, ld, st, tid, T);
	/* cross power: every element read (this row and the mirror row) before any is written */
	constexpr int MX = 8;	/* S <= 8 T (T >= ceil(S / 8)) */
	sg_c64 pv[MX];
#pragma unroll
	for (int it = 0; it < MX; it++) {
		const int ky = tid + it * T;
		if (ky < S && active)
			pv[it] = sg_xpower_at(buf[sg_pad(ky)], oth[sg_pad(ky ? S - ky : 0)], spec[(size_t)row * S + ky]);
	}
	__syncthreads();
#pragma unroll
	for (int it = 0; it < MX; it++) {
		const int ky = tid + it * T;
		if (ky < S && active)
			buf[sg_pad(ky)] = pv[it];
	}
	__syncthreads();
	sg_gen_fft_mixed<false, true>(buf, pl, tw, true, ld, st, tid, T);
}

/* exact sum_n ref(n + k) img(n) (circular) at every candidate k of a near tie (below 2^56) */
__global__ void __launch_bounds__(256)
k_reg_exact(SgSel sel, const int *__restrict__ fa, const int *__restrict__ fb, int ref, int S,
		SgCand *__restrict__ cand) {
	__shared__ unsigned long long part[4];
	const int c = blockIdx.x, slot = blockIdx.y;
	SgCand *cd = cand + slot;
	const unsigned int cnt = cd->count;
	if (cnt > SG_CAND_CAP || (unsigned)c >= cnt)
		return;
	const int frame = (slot & 1) ? fb[slot >> 1] : fa[slot >> 1];
	if (frame < 0)
		return;
	const int k = cd->idx[c], ky = k / S, kx = k - ky * S;
	const uint16_t *R = sel.frame(ref), *I = sel.frame(frame);
	unsigned long long acc = 0;
	for (int y = 0; y < S; y++) {
		const int yr = y + ky < S ? y + ky : y + ky - S;
		const uint16_t *rr = R + (size_t)yr * sel.rp, *ir = I + (size_t)y * sel.rp;
		for (int x = threadIdx.x; x < S; x += blockDim.x) {
			const int xr = x + kx < S ? x + kx : x + kx - S;
			acc += (unsigned long long)((unsigned int)rr[xr] * (unsigned int)ir[x]);
		}
	}
	for (int o = 32; o > 0; o >>= 1)
		acc += __shfl_down(acc, o, 64);
	if ((threadIdx.x & 63) == 0)
		part[threadIdx.x >> 6] = acc;
	__syncthreads();
	if (threadIdx.x == 0)
		cd->exact[c] = (long long)(part[0] + part[1] + part[2] + part[3]);
}

/* a near tie decided by the exact correlations: the largest, lowest index among equals
 * (amb 2 = resolved; 3 = more candidates than SG_CAND_CAP: the FFT arg-max stays) */
__global__ void __launch_bounds__(64)
k_reg_resolve(const SgCand *__restrict__ cand, int S, int np, SgRegOut *__restrict__ out) {
	const int pair = blockIdx.x * blockDim.x + threadIdx.x;
	if (pair >= np)
		return;
	SgRegOut o = out[pair];
	for (int k = 0; k < 2; k++) {
		if (o.amb[k] != 1)
			continue;
		const SgCand *cd = cand + 2 * pair + k;
		const unsigned int cnt = cd->count;
		if (cnt < 1 || cnt > SG_CAND_CAP) {
			o.amb[k] = 3;
			continue;
		}
		int bi = cd->idx[0];
		long long bv = cd->exact[0];
		for (unsigned int c = 1; c < cnt; c++)
			if (cd->exact[c] > bv || (cd->exact[c] == bv && cd->idx[c] < bi)) {
				bv = cd->exact[c];
				bi = cd->idx[c];
			}
		int sy = bi / S, sx = bi % S;
		if (sy > S / 2)
			sy -= S;
		if (sx > S / 2)
			sx -= S;
		o.idx[k] = bi;
		o.sx[k] = sx;
		o.sy[k] = sy;
		o.amb[k] = 2;
	}
	out[pair] = o;
}

/* the estimate's buffers: qbuf (nq subsampled frames, then the frame list), acc [nq][3] + qmax [nq] */
struct SgQBufs {
	uint16_t *qbuf;
	int *frames;
	unsigned long long *acc;
	unsigned int *qmax;
};

static int reg_quality_buffers(sg_ctx *ctx, SgDevice &dv, int nq, int xs, int ys, SgQBufs &qb) {
	if (!dv.aux) {
		HIPCHK(hipStreamCreateWithFlags(&dv.aux, hipStreamNonBlocking));
		for (int k = 0; k < 2; k++)
			HIPCHK(hipEventCreateWithFlags(&dv.aux_ev[k], hipEventDisableTiming));
	}
	if (dv.qacc_h_n < 3 * (size_t)nq) {
		HIPCHK(hipStreamSynchronize(dv.aux));
		if (dv.qacc_h)
			(void)hipHostFree(dv.qacc_h);
		dv.qacc_h = nullptr;
		dv.qacc_h_n = 0;
		HIPCHK(hipHostMalloc((void **)&dv.qacc_h, sizeof(unsigned long long) * 3 * nq));
		dv.qacc_h_n = 3 * (size_t)nq;
	}
	HIPCHK(hipStreamSynchronize(dv.aux));	/* the previous call's buffers are free */
	HIPCHK(ensure(dv.reg_qbuf, (size_t)nq * xs * ys * sizeof(uint16_t) + sizeof(int) * nq + 64));
	HIPCHK(ensure(dv.reg_qacc, (size_t)nq * (3 * sizeof(unsigned long long) + sizeof(unsigned int))));
	qb.qbuf = (uint16_t *)dv.reg_qbuf.p;
	qb.frames = (int *)((char *)dv.reg_qbuf.p + (((size_t)nq * xs * ys * sizeof(uint16_t) + 15) & ~(size_t)15));
	qb.acc = (unsigned long long *)dv.reg_qacc.p;
	qb.qmax = (unsigned int *)(qb.acc + 3 * nq);
	return SG_OK;
}

/* gradient sums of the subsampled frames on the aux stream (after the work queued on it), read
 * back into the pinned block; aux_ev[0] marks them */
static int reg_quality_grad(sg_ctx *ctx, SgDevice &dv, int nq, int xs, int ys, const SgQBufs &qb) {
	const int xb = (int)((double)xs * 0.1) + 1, yb = (int)((double)ys * 0.1) + 1;
	const int wi = xs - 2 * xb, hi = ys - 2 * yb;
	if (wi > 0 && hi > 0) {
		hipLaunchKernelGGL(k_quality_grad_s, dim3((wi + 59) / 60, (hi + SG_QGS_ROWS - 1) / SG_QGS_ROWS, nq), dim3(64), 0,
				dv.aux, qb.qbuf, xs, ys, qb.qmax, qb.acc);
		HIPCHK(hipGetLastError());
	}
	HIPCHK(hipMemcpyAsync(dv.qacc_h, qb.acc, sizeof(unsigned long long) * 3 * nq, hipMemcpyDeviceToHost, dv.aux));
	HIPCHK(hipEventRecord(dv.aux_ev[0], dv.aux));
	return SG_OK;
}

/* The quality estimate of `frames`, enqueued on the device's auxiliary stream (after the work
 * already on `s`, which produced d_sel) so that it runs beside the FFT passes: its kernels are
 * short and the passes leave the chip latency-bound.  reg_quality_finish waits for the sums and
 * forms the values; *launched = false when the subsample loop never runs (dval = 0, :95-98). */
static int reg_quality_launch(sg_ctx *ctx, SgDevice &dv, hipStream_t s, SgSel d_sel, int S,
		const std::vector<int> &frames, bool *launched) {
	*launched = false;
	const int nq = (int)frames.size();
	const int xs = (S - 1) / 3, ys = (S - 1) / 3;
	if (!nq || xs < 2 || ys < 2)
		return SG_OK;
	SgQBufs qb;
	if (int r = reg_quality_buffers(ctx, dv, nq, xs, ys, qb))
		return r;
	HIPCHK(hipEventRecord(dv.aux_ev[1], s));
	HIPCHK(hipStreamWaitEvent(dv.aux, dv.aux_ev[1], 0));
	HIPCHK(hipMemcpyAsync(qb.frames, frames.data(), sizeof(int) * nq, hipMemcpyHostToDevice, dv.aux));
	HIPCHK(hipMemsetAsync(qb.acc, 0, (size_t)nq * (3 * sizeof(unsigned long long) + sizeof(unsigned int)), dv.aux));
	/* one wave per workgroup, walking the row pairs: 283 us per 129 frames of 2048^2 against
	 * 332 / 348 / 403 / 618 us with 128 / 192 / 256 / 384 threads (scripts/gpu_qsub.sh) */
	const int qthr = ctx->knobs.qsub_threads;	/* A/B knob SG_QSUB_THREADS */
	/* the dword loads of k_quality_sub need an even side, even pitches and a dword-aligned base */
	const int al = !(S & 1) && !(d_sel.rp & 1) && !(d_sel.fp & 1) && !((uintptr_t)d_sel.p & 3);
	hipLaunchKernelGGL(k_quality_sub, dim3((ys + SG_QROWS - 1) / SG_QROWS, nq), dim3(qthr), 0, dv.aux, d_sel, al, qb.frames,
			S, xs, ys, qb.qbuf, qb.qmax);
	HIPCHK(hipGetLastError());
	if (int r = reg_quality_grad(ctx, dv, nq, xs, ys, qb))
		return r;
	*launched = true;
	return SG_OK;
}

static int reg_quality_finish(sg_ctx *ctx, SgDevice &dv, int nq, bool launched, std::vector<double> &qual) {
	qual.assign(nq, 0.0);
	if (!launched)
		return SG_OK;
	HIPCHK(hipEventSynchronize(dv.aux_ev[0]));
	const unsigned long long *h = dv.qacc_h;
	for (int i = 0; i < nq; i++) {
		double q;
		if (!h[3 * i + 2]) {
			q = -1.0;
		} else {
			q = (double)h[3 * i] / (double)h[3 * i + 1];
			q = q / 10;
		}
		double dval = 0.0;
		dval += q * 1;
		qual[i] = sqrt(dval);
	}
	return SG_OK;
}

static int reg_dft_device(sg_ctx *ctx, int dev_index, const uint16_t *d_sel_p, int64_t fpitch, int64_t rpitch,
		int nframes, int S, int ref_image, const int *included, int *shiftx, int *shifty, double *quality, void *stream,
		bool normalize_q);

extern "C" int sg_register_dft_u16_device(sg_ctx *ctx, int dev_index, const uint16_t *d_sel, int nframes,
		int S, int ref_image, const int *included, int *shiftx, int *shifty, double *quality,
		void *stream) {
	return reg_dft_device(ctx, dev_index, d_sel, (int64_t)S * S, S, nframes, S, ref_image, included, shiftx, shifty,
			quality, stream, true);
}

extern "C" int sg_register_dft_u16_device_raw(sg_ctx *ctx, int dev_index, const uint16_t *d_sel, int nframes,
		int S, int ref_image, const int *included, int *shiftx, int *shifty, double *quality_raw,
		void *stream) {
	return reg_dft_device(ctx, dev_index, d_sel, (int64_t)S * S, S, nframes, S, ref_image, included, shiftx, shifty,
			quality_raw, stream, false);
}

/* selections read in place from resident frames: selection f row r at d_sel[f frame_pitch + r row_pitch] */
extern "C" int sg_register_dft_u16_device_pitched(sg_ctx *ctx, int dev_index, const uint16_t *d_sel, int64_t frame_pitch,
		int64_t row_pitch, int nframes, int S, int ref_image, const int *included, int *shiftx, int *shifty,
		double *quality, int raw_quality, void *stream) {
	if (ctx && (row_pitch < S || frame_pitch < 0))
		return set_err(ctx, SG_ERR_SIZE, "selection pitches: a row pitch below the side S%s (%ld)", "", (long)row_pitch);
	return reg_dft_device(ctx, dev_index, d_sel, frame_pitch, row_pitch, nframes, S, ref_image, included, shiftx, shifty,
			quality, stream, !raw_quality);
}

/* the plan counts its layouts in these sizes (sg_reg_plan.hpp) */
static_assert(sizeof(SgBest) == SG_REG_SIZEOF_BEST && sizeof(SgRegOut) == SG_REG_SIZEOF_OUT &&
		sizeof(SgCand) == SG_REG_SIZEOF_CAND && sizeof(sg_c64) == SG_REG_SIZEOF_C64 &&
		sizeof(float2) == SG_REG_SIZEOF_C32, "sg_reg_plan.hpp sizes its byte layouts with these");

/* SgRegKernel -> the kernel whose dynamic LDS limit is raised */
static const void *const SG_REG_LDS_KERNELS[SG_RK_COUNT] = {
	(const void *)k_gen_cols_xpower, (const void *)k_gen_rows<true>, (const void *)k_gen_rows<false>,
	(const void *)k_reg_cols<sg_c64, 8>, (const void *)k_reg_rows_fwd_half<sg_c64>,
	(const void *)k_reg_rows_inv_half_argmax<sg_c64, false>, (const void *)k_reg_rows_inv_half_argmax<sg_c64, true>,
	(const void *)k_reg_cols_xpower<sg_c64, 8>, (const void *)k_reg_rows_fwd_half<float2>,
	(const void *)k_reg_rows_inv_half_argmax<float2, false>, (const void *)k_reg_cols<float2, 8>,
	(const void *)k_reg_cols<float2, 16>,
	/* SG_RK_XPOWER32 + SgRegCols32 */
	(const void *)k_reg_cols_xpower<float2, 8, 8>, (const void *)k_reg_cols_xpower<float2, 16>,
	(const void *)k_reg_cols_xpower_w, (const void *)k_reg_cols_fwd_perm_w, (const void *)k_reg_rows_fwd_half_w<false>,
	(const void *)k_reg_rows_fwd_half_w<true>, (const void *)k_reg_rows_inv_half_w};

/* kernel instances with one argument list, indexed by the plan's decisions */
typedef decltype(&k_gen_rows<true>) SgGenRowsFn;
static constexpr SgGenRowsFn SG_GEN_ROWS_KERNELS[2] = {k_gen_rows<false>, k_gen_rows<true>};	/* [bluestein] */
typedef decltype(&k_reg_rows_inv_half_argmax<sg_c64, false>) SgInv64Fn;
static constexpr SgInv64Fn SG_INV64_KERNELS[2] = {	/* [candidates] */
	k_reg_rows_inv_half_argmax<sg_c64, false>, k_reg_rows_inv_half_argmax<sg_c64, true>};
typedef decltype(&k_reg_cols<float2, 8>) SgCols32Fn;
static constexpr SgCols32Fn SG_COLS32_KERNELS[2] = {k_reg_cols<float2, 8>, k_reg_cols<float2, 16>};	/* [ept32 == 16] */
typedef decltype(&k_reg_cols_xpower<float2, 8, 8>) SgXpower32Fn;
static constexpr SgXpower32Fn SG_XPOWER32_KERNELS[2] = {	/* [SgRegCols32]: the block-level forms */
	k_reg_cols_xpower<float2, 8, 8>, k_reg_cols_xpower<float2, 16>};

/* one registration call on its way through the launch steps */
struct SgRegRun {
	sg_ctx *ctx;
	SgDevice &dv;
	hipStream_t s;
	const SgRegPlan &pl;
	SgSel d_sel;
	/* tables (reg_tw, reg_tw32) */
	SgGenTables tbl;
	const sg_c64 *tw;
	const float2 *tw32;
	/* reg_spec: the reference spectrum in fp64, fp32 and (wave-level passes) fp32 lane order;
	 * reg_work: the pair planes (generic path: work2 = the transposed planes) */
	sg_c64 *spec, *work, *work2;
	float2 *spec32, *work32, *specp32;
	/* reg_best: row partials, per-pair results, the pair table and the re-runs' subset of it, the
	 * frames' energies (energy: the main passes, each frame once; energy2: the re-runs'), the
	 * near-tie candidates of one batch, the re-runs' results */
	SgBest *best;
	SgRegOut *d_out, *d_res2;
	int *d_fa, *d_fb, *d_fa2, *d_fb2;
	unsigned long long *energy, *energy2;
	SgCand *cand;
	/* the pinned block: the pair table going up, the results coming back */
	int *pfab;
	SgRegOut *pout;
	std::vector<SgRegOut> hout;	/* the pairs' results on the host */
	SgQBufs qfb;			/* the folded quality estimate's buffers */
	bool ref_pending;	/* set by reg_ref_spectrum32 (the spectrum is on its own stream); cleared by the first reg_half32, which waits for it, or behind the batch loop */
	bool q_fold_last;	/* set by reg_main_batches for every batch (true on the last); read by reg_half32: the gradient follows */
	int q_qbase;		/* set by reg_main_batches for every batch (its first frame's entry of qframes); read by reg_half32 */
	bool q_launched;	/* set by reg_quality_launch or reg_half32's gradient, never cleared; read by reg_quality_readback */
};

/* tables: twiddles exp(-2 pi i k / S); generic path: for Bluestein the m-point twiddles, the
 * chirp c_j = exp(-i pi j^2 / S) and FFT_m(b).  They depend on S (and the path) only: uploaded
 * when either changes */
static int reg_upload_tables64(SgRegRun &r) {
	sg_ctx *ctx = r.ctx;
	SgDevice &dv = r.dv;
	const SgRegPlan &pl = r.pl;
	const bool blue = pl.gen.bluestein != 0;
	if (dv.reg_tab_S != pl.S || dv.reg_tab_generic != (int)pl.generic) {
		std::vector<double> tw, twm, ch, bh;
		make_twiddles(pl.S, tw);
		if (blue) {
			make_twiddles(pl.gen.m, twm);
			make_bluestein(pl.S, (size_t)pl.gen.m, ch, bh);
		}
		dv.reg_tab_S = 0;
		HIPCHK(ensure(dv.reg_tw, sizeof(double) * pl.tab_total));
		double *d = (double *)dv.reg_tw.p;
		HIPCHK(hipMemcpyAsync(d, tw.data(), sizeof(double) * pl.n_tw, hipMemcpyHostToDevice, r.s));
		if (blue) {
			HIPCHK(hipMemcpyAsync(d + pl.n_tw, twm.data(), sizeof(double) * pl.n_twm, hipMemcpyHostToDevice, r.s));
			HIPCHK(hipMemcpyAsync(d + pl.n_tw + pl.n_twm, ch.data(), sizeof(double) * pl.n_ch, hipMemcpyHostToDevice, r.s));
			HIPCHK(hipMemcpyAsync(d + pl.n_tw + pl.n_twm + pl.n_ch, bh.data(), sizeof(double) * pl.n_bh,
					hipMemcpyHostToDevice, r.s));
		}
		HIPCHK(hipStreamSynchronize(r.s));	/* the host vectors die here */
		dv.reg_tab_S = pl.S;
		dv.reg_tab_generic = (int)pl.generic;
	}
	double *d = (double *)dv.reg_tw.p;
	memset(&r.tbl, 0, sizeof r.tbl);
	r.tbl.tw = (const sg_c64 *)d;
	if (blue) {
		r.tbl.twm = (const sg_c64 *)(d + pl.n_tw);
		r.tbl.chirp = (const sg_c64 *)(d + pl.n_tw + pl.n_twm);
		r.tbl.bhat = (const sg_c64 *)(d + pl.n_tw + pl.n_twm + pl.n_ch);
	}
	r.tw = r.tbl.tw;
	return SG_OK;
}

/* fp32 twiddles, rounded from the fp64 table; uploaded when S changes */
static int reg_upload_tables32(SgRegRun &r) {
	sg_ctx *ctx = r.ctx;
	SgDevice &dv = r.dv;
	r.tw32 = nullptr;
	if (!r.pl.fp32)
		return SG_OK;
	if (dv.reg_tw32_S != r.pl.S) {
		dv.reg_tw32_S = 0;
		HIPCHK(ensure(dv.reg_tw32, 2 * (size_t)r.pl.S * sizeof(float2)));
		std::vector<float> t32;
		make_twiddles32(r.pl.S, t32);
		HIPCHK(hipMemcpyAsync(dv.reg_tw32.p, t32.data(), sizeof(float) * t32.size(), hipMemcpyHostToDevice, r.s));
		HIPCHK(hipStreamSynchronize(r.s));
		dv.reg_tw32_S = r.pl.S;
	}
	r.tw32 = (const float2 *)dv.reg_tw32.p;
	return SG_OK;
}

static void reg_raise_lds(const SgRegPlan &pl) {
	for (const SgRegLdsAttr &a : pl.lds_attrs)
		(void)hipFuncSetAttribute(SG_REG_LDS_KERNELS[a.kernel], hipFuncAttributeMaxDynamicSharedMemorySize, a.bytes);
}

/* device workspace: reg_spec, reg_work and reg_best carved at the plan's offsets, the energies zeroed */
static int reg_carve_workspace(SgRegRun &r) {
	sg_ctx *ctx = r.ctx;
	SgDevice &dv = r.dv;
	const SgRegPlan &pl = r.pl;
	const int NP = pl.NP;
	HIPCHK(ensure(dv.reg_spec, pl.spec_bytes));
	HIPCHK(ensure(dv.reg_work, pl.work_bytes));
	HIPCHK(ensure(dv.reg_best, pl.ws));
	char *wsp = (char *)dv.reg_best.p;
	r.spec = (sg_c64 *)dv.reg_spec.p;
	r.work = (sg_c64 *)dv.reg_work.p;
	r.spec32 = (float2 *)((char *)dv.reg_spec.p + pl.plane * sizeof(sg_c64));
	r.work32 = (float2 *)dv.reg_work.p;
	r.specp32 = pl.specp_on ? r.spec32 + pl.plane : nullptr;
	r.work2 = r.work + (size_t)pl.Bc * pl.plane;	/* generic path: transposed planes */
	r.best = (SgBest *)wsp;
	r.d_out = (SgRegOut *)(wsp + pl.o_out);
	r.d_res2 = (SgRegOut *)(wsp + pl.o_res2);
	r.d_fa = (int *)(wsp + pl.o_fab);
	r.d_fb = r.d_fa + (NP + 1);
	r.d_fa2 = r.d_fb + (NP + 1);
	r.d_fb2 = r.d_fa2 + (NP + 1);
	r.energy = (unsigned long long *)(wsp + pl.o_en);
	r.energy2 = r.energy + pl.nframes;
	r.cand = (SgCand *)(wsp + pl.o_cand);
	HIPCHK(hipMemsetAsync(r.energy, 0, sizeof(unsigned long long) * 2 * pl.nframes, r.s));
	return SG_OK;
}

/* aux2: the stream of an fp32 call's reference spectrum */
static int reg_ref_stream(SgRegRun &r) {
	sg_ctx *ctx = r.ctx;
	SgDevice &dv = r.dv;
	if (r.pl.fp32 && !dv.aux2) {
		HIPCHK(hipStreamCreateWithFlags(&dv.aux2, hipStreamNonBlocking));
		for (int k = 0; k < 2; k++)
			HIPCHK(hipEventCreateWithFlags(&dv.aux2_ev[k], hipEventDisableTiming));
	}
	return SG_OK;
}

/* the pair table goes up, and the results come back, through a pinned block (the previous
 * call's copies are done: every call ends on a stream synchronize) */
static int reg_upload_pairs(SgRegRun &r) {
	sg_ctx *ctx = r.ctx;
	SgDevice &dv = r.dv;
	const SgRegPlan &pl = r.pl;
	const int NP = pl.NP;
	r.hout.resize((size_t)NP);
	if (dv.reg_pin_n < pl.pin_bytes) {
		if (dv.reg_pin)
			(void)hipHostFree(dv.reg_pin);
		dv.reg_pin = nullptr;
		dv.reg_pin_n = 0;
		HIPCHK(hipHostMalloc(&dv.reg_pin, pl.pin_bytes));
		dv.reg_pin_n = pl.pin_bytes;
	}
	r.pfab = (int *)dv.reg_pin;
	r.pout = (SgRegOut *)((char *)dv.reg_pin + pl.pin_res);
	memcpy(r.pfab, pl.hfa.data(), sizeof(int) * (NP + 1));
	memcpy(r.pfab + (NP + 1), pl.hfb.data(), sizeof(int) * (NP + 1));
	HIPCHK(hipMemcpyAsync(r.d_fa, r.pfab, sizeof(int) * 2 * (NP + 1), hipMemcpyHostToDevice, r.s));	/* d_fb = d_fa + NP + 1 */
	return SG_OK;
}

/* the quality estimate on the aux stream, queued behind the main stream's table uploads and
 * fills (queued ahead of them, its long-running workgroups held the fills' single workgroup
 * back 0.2 ms, profiles/r05m_*) */
static int reg_quality_start(SgRegRun &r) {
	sg_ctx *ctx = r.ctx;
	const SgRegPlan &pl = r.pl;
	if (pl.qroute == SG_REG_Q_FOLDED) {	/* the sums zeroed on the call's stream, ahead of every forward row launch */
		const int nq = (int)pl.qframes.size(), xs = (pl.S - 1) / 3;
		if (int rc = reg_quality_buffers(ctx, r.dv, nq, xs, xs, r.qfb))
			return rc;
		HIPCHK(hipMemsetAsync(r.qfb.acc, 0, (size_t)nq * (3 * sizeof(unsigned long long) + sizeof(unsigned int)), r.s));
		return SG_OK;
	}
	return reg_quality_launch(ctx, r.dv, r.s, r.d_sel, pl.S, pl.qframes, &r.q_launched);
}

/* the generic row kernel over np pairs' rows of `data` */
static void reg_gen_rows(const SgRegRun &r, const int *fa, const int *fb, int np, sg_c64 *data, int mode, int inverse,
		unsigned long long *en, const SgRegOut *res, SgCand *cand) {
	const SgRegPlan &pl = r.pl;
	hipLaunchKernelGGL(SG_GEN_ROWS_KERNELS[pl.gen.bluestein], dim3(pl.S, np), dim3(pl.gen_thr), pl.gen_lds, r.s, r.d_sel,
			fa, fb, data, pl.S, pl.gen, r.tbl, mode, inverse, en, r.best, res, cand);
}

/* the wave-level forward rows of np pairs (or, np = 1, of the reference) into `out` */
static void reg_fwd_w_launch(const SgRegRun &r, hipStream_t st, const int *fa, const int *fb, int np, float2 *out,
		unsigned long long *en, int rows, int qbase) {
	const SgRegPlan &pl = r.pl;
	const int S = pl.S, qfold = pl.qfold;
	if (qfold) {
		const int waves = (S + qfold - 1) / qfold;
		hipLaunchKernelGGL(k_reg_rows_fwd_half_w<true>, dim3((waves + 3) / 4, np), dim3(256), pl.wcol_lds, st, r.d_sel, fa,
				fb, r.tw32, out, en, qfold, r.qfb.qbuf, r.qfb.qmax, qbase);
	} else {
		hipLaunchKernelGGL(k_reg_rows_fwd_half_w<false>, dim3(S / 4 / rows, np), dim3(256), pl.wcol_lds, st, r.d_sel, fa,
				fb, r.tw32, out, en, rows, (uint16_t *)nullptr, (unsigned int *)nullptr, 0);
	}
}

/* fp64 reference spectrum of the half-spectrum passes, its energy into `en` */
static int reg_ref_spectrum64(SgRegRun &r, unsigned long long *en) {
	sg_ctx *ctx = r.ctx;
	const SgRegPlan &pl = r.pl;
	const int S = pl.S, NP = pl.NP;
	hipLaunchKernelGGL(k_reg_rows_fwd_half<sg_c64>, dim3(S / pl.rpb, 1), dim3(pl.row_thr), pl.row_lds, r.s, r.d_sel,
			r.d_fa + NP, r.d_fb + NP, S, r.tw, r.spec, en, pl.rpb);
	HIPCHK(hipGetLastError());
	hipLaunchKernelGGL((k_reg_cols<sg_c64, 8>), dim3(S / 2 / pl.CWh, 1), dim3(pl.colh_thr), pl.colh_lds, r.s, r.spec, S,
			pl.logS, pl.CWh, r.tw, 0);
	HIPCHK(hipGetLastError());
	return SG_OK;
}

/* fp32 reference spectrum on its own stream beside the first batch's forward rows (which do
 * not read it; the batch's column pass waits for it).  One workgroup per CU at most: run
 * alone it is 0.27 ms of latency-bound passes ahead of every pair (profiles/r05l_*) */
static int reg_ref_spectrum32(SgRegRun &r) {
	sg_ctx *ctx = r.ctx;
	SgDevice &dv = r.dv;
	const SgRegPlan &pl = r.pl;
	const int S = pl.S, NP = pl.NP;
	const hipStream_t rs = dv.aux2;
	HIPCHK(hipEventRecord(dv.aux2_ev[0], r.s));
	HIPCHK(hipStreamWaitEvent(rs, dv.aux2_ev[0], 0));
	if (r.specp32) {	/* wave-level passes: one row per wave, the columns straight into lane order */
		reg_fwd_w_launch(r, rs, r.d_fa + NP, r.d_fb + NP, 1, r.spec32, r.energy, 1, 0);
		HIPCHK(hipGetLastError());
		hipLaunchKernelGGL(k_reg_cols_fwd_perm_w, dim3(S / 2 / 4), dim3(256), pl.wcol_lds, rs, r.spec32, r.specp32, r.tw32);
	} else {
		hipLaunchKernelGGL(k_reg_rows_fwd_half<float2>, dim3(S / pl.rpb, 1), dim3(pl.row_thr), pl.row_lds32, rs, r.d_sel,
				r.d_fa + NP, r.d_fb + NP, S, r.tw32, r.spec32, r.energy, pl.rpb);
		HIPCHK(hipGetLastError());
		hipLaunchKernelGGL(SG_COLS32_KERNELS[pl.ept32 == 16], dim3(S / 2 / pl.CW32, 1), dim3(pl.colh_thr32), pl.colh_lds32,
				rs, r.spec32, S, pl.logS, pl.CW32, r.tw32, 0);
	}
	HIPCHK(hipGetLastError());
	HIPCHK(hipEventRecord(dv.aux2_ev[1], rs));
	r.ref_pending = true;
	return SG_OK;
}

/* generic reference spectrum: rows, transpose, rows (transposed layout) */
static int reg_ref_spectrum_gen(SgRegRun &r) {
	sg_ctx *ctx = r.ctx;
	const SgRegPlan &pl = r.pl;
	const int NP = pl.NP;
	reg_gen_rows(r, r.d_fa + NP, r.d_fb + NP, 1, r.work, (int)SG_GEN_FWD_U16, 0, r.energy, nullptr, nullptr);
	HIPCHK(hipGetLastError());
	hipLaunchKernelGGL(k_gen_transpose, dim3(pl.tgrid, pl.tgrid, 1), dim3(32, 8), 0, r.s, (const sg_c64 *)r.work, r.spec,
			pl.S);
	HIPCHK(hipGetLastError());
	reg_gen_rows(r, r.d_fa + NP, r.d_fb + NP, 1, r.spec, (int)SG_GEN_C2C, 0, r.energy, nullptr, nullptr);
	HIPCHK(hipGetLastError());
	return SG_OK;
}

/* generic passes up to the cross power's inverse: transposed spectrum of the rows of `fa`
 * / `fb` pairs -> `work` holds the pairs' inverse column transforms in row layout */
static int reg_gen_forward(SgRegRun &r, const int *fa, const int *fb, int np, unsigned long long *en) {
	sg_ctx *ctx = r.ctx;
	const SgRegPlan &pl = r.pl;
	const int S = pl.S;
	const dim3 tgrid(pl.tgrid, pl.tgrid, np);
	reg_gen_rows(r, fa, fb, np, r.work, (int)SG_GEN_FWD_U16, 0, en, nullptr, nullptr);
	HIPCHK(hipGetLastError());
	hipLaunchKernelGGL(k_gen_transpose, tgrid, dim3(32, 8), 0, r.s, (const sg_c64 *)r.work, r.work2, S);
	HIPCHK(hipGetLastError());
	if (pl.gen_fuse) {	/* forward columns + cross power + inverse columns in one pass */
		hipLaunchKernelGGL(k_gen_cols_xpower, dim3(S / 2 + 1, np), dim3(2 * pl.gen_thr), 2 * pl.gen_lds, r.s, r.work2,
				(const sg_c64 *)r.spec, S, pl.gen, r.tw);
		HIPCHK(hipGetLastError());
	} else {
		reg_gen_rows(r, fa, fb, np, r.work2, (int)SG_GEN_C2C, 0, en, nullptr, nullptr);
		HIPCHK(hipGetLastError());
		hipLaunchKernelGGL(k_gen_xpower, dim3(1024, np), dim3(256), 0, r.s, r.work2, (const sg_c64 *)r.spec, S);
		HIPCHK(hipGetLastError());
		reg_gen_rows(r, fa, fb, np, r.work2, (int)SG_GEN_C2C, 1, en, nullptr, nullptr);
		HIPCHK(hipGetLastError());
	}
	hipLaunchKernelGGL(k_gen_transpose, tgrid, dim3(32, 8), 0, r.s, (const sg_c64 *)r.work2, r.work, S);
	HIPCHK(hipGetLastError());
	return SG_OK;
}

/* fp64 half-spectrum passes of the pairs (fa, fb)[0, np) against the fp64 reference spectrum:
 * `cand` 0 = top-2 arg-max into best, 1 = near-tie candidates of the results `res` */
static int reg_half64(SgRegRun &r, const int *fa, const int *fb, int np, unsigned long long *en, int cand,
		const SgRegOut *res) {
	sg_ctx *ctx = r.ctx;
	const SgRegPlan &pl = r.pl;
	const int S = pl.S;
	hipLaunchKernelGGL(k_reg_rows_fwd_half<sg_c64>, dim3(S / pl.rpb, np), dim3(pl.row_thr), pl.row_lds, r.s, r.d_sel, fa, fb,
			S, r.tw, r.work, en, pl.rpb);
	HIPCHK(hipGetLastError());
	hipLaunchKernelGGL((k_reg_cols_xpower<sg_c64, 8>), dim3(S / pl.CWh, np), dim3(pl.colh_thr), pl.colh_lds, r.s, r.work,
			(const sg_c64 *)r.spec, S, pl.CWh, r.tw);
	HIPCHK(hipGetLastError());
	hipLaunchKernelGGL(SG_INV64_KERNELS[cand], dim3(S, np), dim3(pl.row_thr), pl.row_lds, r.s, (const sg_c64 *)r.work, S,
			r.tw, r.best, cand ? res : (const SgRegOut *)nullptr, cand ? r.cand : (SgCand *)nullptr);
	HIPCHK(hipGetLastError());
	return SG_OK;
}

/* what the first / last batch's fp32 forward rows are followed by: the wait for the reference
 * spectrum's stream, the folded estimate's gradient */
static int reg_half32_after_rows(SgRegRun &r) {
	sg_ctx *ctx = r.ctx;
	SgDevice &dv = r.dv;
	const SgRegPlan &pl = r.pl;
	if (r.ref_pending) {	/* the reference spectrum, from its stream */
		HIPCHK(hipStreamWaitEvent(r.s, dv.aux2_ev[1], 0));
		r.ref_pending = false;
	}
	if (pl.qfold && r.q_fold_last) {	/* every frame subsampled (the reference's rows waited for above) */
		const int nq = (int)pl.qframes.size(), xs = (pl.S - 1) / 3;
		HIPCHK(hipEventRecord(dv.aux_ev[1], r.s));
		HIPCHK(hipStreamWaitEvent(dv.aux, dv.aux_ev[1], 0));
		if (int rc = reg_quality_grad(ctx, dv, nq, xs, xs, r.qfb))
			return rc;
		r.q_launched = true;
	}
	return SG_OK;
}

/* fp32 half-spectrum passes of the pairs (fa, fb)[0, np): top-2 arg-max into best */
static int reg_half32(SgRegRun &r, const int *fa, const int *fb, int np, unsigned long long *en) {
	sg_ctx *ctx = r.ctx;
	const SgRegPlan &pl = r.pl;
	const int S = pl.S;
	if (pl.wcol)
		reg_fwd_w_launch(r, r.s, fa, fb, np, r.work32, en, pl.rpw, r.q_qbase);
	else
		hipLaunchKernelGGL(k_reg_rows_fwd_half<float2>, dim3(S / pl.rpb, np), dim3(pl.row_thr), pl.row_lds32, r.s, r.d_sel,
				fa, fb, S, r.tw32, r.work32, en, pl.rpb);
	HIPCHK(hipGetLastError());
	if (int rc = reg_half32_after_rows(r))
		return rc;
	if (pl.cols32 == SG_COLS32_WAVE8_PERM) {	/* S = 2048: the wave-level column pass (SG_REG_WCOL=0: the block-level one, A/B), 8-column strips: 64-B row segments, one workgroup per CU */
		hipLaunchKernelGGL(k_reg_cols_xpower_w, dim3(S / 8, np), dim3(64 * 8), 2 * pl.wcol_lds, r.s, r.work32,
				(const float2 *)r.spec32, (const float2 *)r.specp32, r.tw32);
	} else {	/* 8 elements per thread at 64 VGPRs, or 16 */
		hipLaunchKernelGGL(SG_XPOWER32_KERNELS[pl.cols32], dim3(S / pl.CW32, np), dim3(pl.colh_thr32), pl.colh_lds32, r.s,
				r.work32, (const float2 *)r.spec32, S, pl.CW32, r.tw32);
	}
	HIPCHK(hipGetLastError());
	if (pl.wcol)
		hipLaunchKernelGGL(k_reg_rows_inv_half_w, dim3(S / 4, np), dim3(256), pl.wcol_lds, r.s, (const float2 *)r.work32,
				r.tw32, r.best);
	else
		hipLaunchKernelGGL((k_reg_rows_inv_half_argmax<float2, false>), dim3(S, np), dim3(pl.row_thr), pl.row_lds32, r.s,
				(const float2 *)r.work32, S, r.tw32, r.best, (const SgRegOut *)nullptr, (SgCand *)nullptr);
	HIPCHK(hipGetLastError());
	return SG_OK;
}

/* reference spectrum R = FFT2(ref) (half layout: the A' half only; generic: transposed) */
static int reg_ref_spectrum(SgRegRun &r) {
	if (r.pl.generic)
		return reg_ref_spectrum_gen(r);
	if (r.pl.fp32)
		return reg_ref_spectrum32(r);
	return reg_ref_spectrum64(r, r.energy);
}

/* the pairs in batches of B: their passes, then per pair the shifts and the near-tie flags;
 * the results come back through the pinned block */
static int reg_main_batches(SgRegRun &r) {
	sg_ctx *ctx = r.ctx;
	const SgRegPlan &pl = r.pl;
	const int S = pl.S, npairs_total = pl.npairs_total;
	for (int p0 = 0; p0 < npairs_total; p0 += pl.B) {
		const int np = npairs_total - p0 < pl.B ? npairs_total - p0 : pl.B;
		if (pl.generic) {
			if (int rc = reg_gen_forward(r, r.d_fa + p0, r.d_fb + p0, np, r.energy))
				return rc;
			reg_gen_rows(r, r.d_fa + p0, r.d_fb + p0, np, r.work, (int)SG_GEN_INV_ARGMAX, 1, r.energy, nullptr, nullptr);
		} else if (pl.fp32) {
			r.q_qbase = 1 + 2 * p0;	/* qframes = ref, todo...: pair k's frames are entries 1 + 2k, 2 + 2k */
			r.q_fold_last = p0 + np >= npairs_total;
			if (int rc = reg_half32(r, r.d_fa + p0, r.d_fb + p0, np, r.energy))
				return rc;
		} else {
			if (int rc = reg_half64(r, r.d_fa + p0, r.d_fb + p0, np, r.energy, 0, nullptr))
				return rc;
		}
		HIPCHK(hipGetLastError());
		hipLaunchKernelGGL(k_reg_final, dim3(np), dim3(256), 0, r.s, (const SgBest *)r.best, S, S /* row partials per pair */,
				(const int *)r.d_fa + p0, (const int *)r.d_fb + p0, pl.ref_image, (const unsigned long long *)r.energy,
				pl.tol_main, r.d_out + p0);
		HIPCHK(hipGetLastError());
	}
	if (r.ref_pending) {
		HIPCHK(hipStreamWaitEvent(r.s, r.dv.aux2_ev[1], 0));
		r.ref_pending = false;
	}
	if (npairs_total > 0)
		HIPCHK(hipMemcpyAsync(r.pout, r.d_out, sizeof(SgRegOut) * npairs_total, hipMemcpyDeviceToHost, r.s));
	HIPCHK(hipStreamSynchronize(r.s));
	if (npairs_total > 0)
		memcpy(r.hout.data(), r.pout, sizeof(SgRegOut) * npairs_total);
	return SG_OK;
}

/* the pairs with a near tie (the runner-up within the tolerance of the maximum) */
static void reg_ambiguous(const SgRegRun &r, std::vector<int> &amb) {
	amb.clear();
	for (int k = 0; k < r.pl.npairs_total; k++)
		if (r.hout[k].amb[0] == 1 || r.hout[k].amb[1] == 1)
			amb.push_back(k);
}

/* the pairs `amb` and their results so far as a pair table of their own (d_fa2, d_fb2, d_res2) */
static int reg_upload_subset(SgRegRun &r, const std::vector<int> &amb, std::vector<SgRegOut> &ares) {
	sg_ctx *ctx = r.ctx;
	const int na = (int)amb.size();
	std::vector<int> afa(na), afb(na);
	ares.resize(na);
	for (int i = 0; i < na; i++) {
		afa[i] = r.pl.hfa[amb[i]];
		afb[i] = r.pl.hfb[amb[i]];
		ares[i] = r.hout[amb[i]];
	}
	HIPCHK(hipMemcpyAsync(r.d_fa2, afa.data(), sizeof(int) * na, hipMemcpyHostToDevice, r.s));
	HIPCHK(hipMemcpyAsync(r.d_fb2, afb.data(), sizeof(int) * na, hipMemcpyHostToDevice, r.s));
	HIPCHK(hipMemcpyAsync(r.d_res2, ares.data(), sizeof(SgRegOut) * na, hipMemcpyHostToDevice, r.s));
	HIPCHK(hipStreamSynchronize(r.s));	/* the host vectors die here */
	return SG_OK;
}

/* the subset's results back into the pairs' */
static int reg_download_subset(SgRegRun &r, const std::vector<int> &amb, std::vector<SgRegOut> &ares) {
	sg_ctx *ctx = r.ctx;
	const int na = (int)amb.size();
	HIPCHK(hipMemcpyAsync(ares.data(), r.d_res2, sizeof(SgRegOut) * na, hipMemcpyDeviceToHost, r.s));
	HIPCHK(hipStreamSynchronize(r.s));
	for (int i = 0; i < na; i++)
		r.hout[amb[i]] = ares[i];
	return SG_OK;
}

/* near ties after fp32 passes: the fp64 reference spectrum, then the pairs' fp64 passes and a
 * fresh arg-max at the fp64 tolerance */
static int reg_rerun_fp64(SgRegRun &r, std::vector<int> &amb, std::vector<SgRegOut> &ares) {
	sg_ctx *ctx = r.ctx;
	const SgRegPlan &pl = r.pl;
	if (int rc = reg_upload_subset(r, amb, ares))
		return rc;
	if (int rc = reg_ref_spectrum64(r, r.energy2))
		return rc;
	const int na = (int)amb.size();
	for (int p0 = 0; p0 < na; p0 += pl.B64) {
		const int np = na - p0 < pl.B64 ? na - p0 : pl.B64;
		if (int rc = reg_half64(r, r.d_fa2 + p0, r.d_fb2 + p0, np, r.energy2, 0, nullptr))
			return rc;
		/* `energy`, not `energy2`, on purpose: the tolerance takes each frame's sum of squares once,
		 * which the main passes left in energy.  energy2 only keeps the re-runs' forward rows from
		 * adding the same rows to energy a second time (a frame re-run here and again for its
		 * candidates has twice its energy there); no kernel reads it */
		hipLaunchKernelGGL(k_reg_final, dim3(np), dim3(256), 0, r.s, (const SgBest *)r.best, pl.S, pl.S,
				(const int *)r.d_fa2 + p0, (const int *)r.d_fb2 + p0, pl.ref_image, (const unsigned long long *)r.energy,
				-32, r.d_res2 + p0);
		HIPCHK(hipGetLastError());
	}
	if (int rc = reg_download_subset(r, amb, ares))
		return rc;
	r.dv.stats.reg_fp64_reruns += (uint64_t)na;
	reg_ambiguous(r, amb);
	return SG_OK;
}

/* what is still a near tie in fp64: every index within the tolerance is listed, their exact
 * integer correlations computed and the largest taken (lowest index among exact equals) */
static int reg_resolve_exact(SgRegRun &r, const std::vector<int> &amb, std::vector<SgRegOut> &ares) {
	sg_ctx *ctx = r.ctx;
	const SgRegPlan &pl = r.pl;
	const int S = pl.S;
	if (int rc = reg_upload_subset(r, amb, ares))
		return rc;
	const int na = (int)amb.size();
	for (int p0 = 0; p0 < na; p0 += pl.B64) {
		const int np = na - p0 < pl.B64 ? na - p0 : pl.B64;
		HIPCHK(hipMemsetAsync(r.cand, 0, sizeof(SgCand) * 2 * np, r.s));
		if (pl.generic) {
			if (int rc = reg_gen_forward(r, r.d_fa2 + p0, r.d_fb2 + p0, np, r.energy2))
				return rc;
			reg_gen_rows(r, r.d_fa2 + p0, r.d_fb2 + p0, np, r.work, (int)SG_GEN_INV_CAND, 1, r.energy2,
					(const SgRegOut *)(r.d_res2 + p0), r.cand);
		} else {
			/* the fp64 spectrum exists on the fp64 half path, and after the fp64 re-run */
			if (int rc = reg_half64(r, r.d_fa2 + p0, r.d_fb2 + p0, np, r.energy2, 1, (const SgRegOut *)(r.d_res2 + p0)))
				return rc;
		}
		HIPCHK(hipGetLastError());
		hipLaunchKernelGGL(k_reg_exact, dim3(SG_CAND_CAP, 2 * np), dim3(256), 0, r.s, r.d_sel, (const int *)r.d_fa2 + p0,
				(const int *)r.d_fb2 + p0, pl.ref_image, S, r.cand);
		HIPCHK(hipGetLastError());
		hipLaunchKernelGGL(k_reg_resolve, dim3((np + 63) / 64), dim3(64), 0, r.s, (const SgCand *)r.cand, S, np,
				r.d_res2 + p0);
		HIPCHK(hipGetLastError());
	}
	return reg_download_subset(r, amb, ares);
}

/* the pairs' shifts to their frames, and the call's tie statistics */
static void reg_scatter_shifts(SgRegRun &r, int *shiftx, int *shifty) {
	for (int k = 0; k < r.pl.npairs_total; k++) {
		const int fr[2] = {r.pl.hfa[k], r.pl.hfb[k]};
		for (int h = 0; h < 2; h++) {
			if (fr[h] < 0)
				continue;
			shiftx[fr[h]] = r.hout[k].sx[h];
			shifty[fr[h]] = r.hout[k].sy[h];
			if (r.hout[k].amb[h] == 2)
				r.dv.stats.reg_ties_resolved++;
			else if (r.hout[k].amb[h])
				r.dv.stats.reg_ties_unresolved++;
		}
	}
}

/* the end of the call's device span, the quality values, and (normalize_q) their normalisation */
static int reg_quality_readback(SgRegRun &r, const int *included, double *quality, bool normalize_q) {
	sg_ctx *ctx = r.ctx;
	SgDevice &dv = r.dv;
	const SgRegPlan &pl = r.pl;
	const std::vector<int> &todo = pl.todo;
	std::vector<double> qual;
	if (r.q_launched)	/* the span ends with the quality estimate's stream */
		HIPCHK(hipStreamWaitEvent(r.s, dv.aux_ev[0], 0));
	HIPCHK(hipEventRecord(dv.ev[1], r.s));
	if (int qrc = reg_quality_finish(ctx, dv, (int)pl.qframes.size(), r.q_launched, qual))
		return qrc;
	{
		float ms = 0.f;
		HIPCHK(hipEventSynchronize(dv.ev[1]));
		HIPCHK(hipEventElapsedTime(&ms, dv.ev[0], dv.ev[1]));
		dv.stats.reg_ms = ms;
	}
	/* quality: q_min/q_max seeded by the reference frame, then frames in index order with
	 * the reference's min() macro (src/core/siril.h), then normalizeQualityData */
	if (!normalize_q) {	/* raw values of the processed frames (sharded registration) */
		quality[pl.ref_image] = qual[0];
		for (size_t k = 0; k < todo.size(); k++)
			quality[todo[k]] = qual[k + 1];
		return SG_OK;
	}
	double q_min = qual[0], q_max = qual[0];
	quality[pl.ref_image] = qual[0];
	for (size_t k = 0; k < todo.size(); k++) {
		const double qv = qual[k + 1];
		quality[todo[k]] = qv;
		if (qv > q_max)
			q_max = qv;
		q_min = (q_min < qv) ? q_min : qv;
	}
	for (int f = 0; f < pl.nframes; f++) {
		if (included && !included[f])
			continue;
		quality[f] -= q_min;
		quality[f] /= (q_max - q_min);
	}
	return SG_OK;
}

/* tables, LDS limits, workspace and pair table of a planned call, then the quality estimate (or
 * the folded one's zeroed sums) and the reference spectrum */
static int reg_setup(SgRegRun &r) {
	sg_ctx *ctx = r.ctx;
	if (int rc = reg_upload_tables64(r))
		return rc;
	HIPCHK(hipEventRecord(r.dv.ev[0], r.s));	/* the call's device span (sg_stack_stats.reg_ms) */
	reg_raise_lds(r.pl);
	if (int rc = reg_carve_workspace(r))
		return rc;
	if (int rc = reg_upload_tables32(r))
		return rc;
	if (int rc = reg_ref_stream(r))
		return rc;
	if (int rc = reg_upload_pairs(r))
		return rc;
	if (int rc = reg_quality_start(r))
		return rc;
	return reg_ref_spectrum(r);
}

static int reg_dft_device(sg_ctx *ctx, int dev_index, const uint16_t *d_sel_p, int64_t fpitch, int64_t rpitch,
		int nframes, int S, int ref_image, const int *included, int *shiftx, int *shifty, double *quality, void *stream,
		bool normalize_q) {
	if (!ctx || dev_index < 0 || dev_index >= (int)ctx->dev.size() || !d_sel_p || !shiftx || !shifty || !quality)
		return SG_ERR_GENERIC;
	SgRegPlan pl;
	if (int rc = sg_reg_plan(nframes, S, ref_image, included, fpitch, rpitch, ctx->knobs, pl))
		return set_err(ctx, rc, "%s%.0ld", pl.err, 0);
	SgDevice &dv = ctx->dev[dev_index];
	HIPCHK(hipSetDevice(dv.id));
	/* the call's tie statistics: the device's record (one host thread per device), published to
	 * the context when the call returns */
	dv.stats.reg_ties_resolved = dv.stats.reg_ties_unresolved = dv.stats.reg_fp64_reruns = 0;
	dv.stats.reg_ms = 0.0;
	struct Publish {
		sg_ctx *c;
		const sg_stack_stats &s;
		~Publish() {
			std::lock_guard<std::mutex> lk(c->mu);
			c->stats.reg_ties_resolved = s.reg_ties_resolved;
			c->stats.reg_ties_unresolved = s.reg_ties_unresolved;
			c->stats.reg_fp64_reruns = s.reg_fp64_reruns;
			c->stats.reg_ms = s.reg_ms;
		}
	} publish{ctx, dv.stats};
	SgRegRun r{ctx, dv, stream ? (hipStream_t)stream : dv.stream, pl, SgSel{d_sel_p, (long long)pl.fpitch, (long long)pl.rpitch}};
	if (int rc = reg_setup(r))
		return rc;
	shiftx[pl.ref_image] = 0;
	shifty[pl.ref_image] = 0;
	if (int rc = reg_main_batches(r))
		return rc;
	/* near ties: re-run those pairs.  After fp32 passes, first in fp64; what is still a near tie
	 * then goes to the exact integer correlations */
	std::vector<int> amb;
	std::vector<SgRegOut> ares;
	reg_ambiguous(r, amb);
	if (!amb.empty() && pl.fp32)
		if (int rc = reg_rerun_fp64(r, amb, ares))
			return rc;
	if (!amb.empty())
		if (int rc = reg_resolve_exact(r, amb, ares))
			return rc;
	reg_scatter_shifts(r, shiftx, shifty);
	return reg_quality_readback(r, included, quality, normalize_q);
}

/*
 * host selections: one device registers everything; several devices split the frames to
 * register into contiguous shards (frames are independent), each device driven by
 * its own host thread with the reference selection and its shard uploaded, the reference
 * spectrum and quality computed on every device.  The raw shard results are reassembled and
 * the quality bookkeeping of the reference (q_min / q_max seeded by the reference frame, the
 * frames in index order, the min() macro, normalizeQualityData :163-176) replayed over all of
 * them, so the result is the one-device result (test_register_raw_shards_reassemble).
 */
static int reg_host(sg_ctx *ctx, const uint16_t *sel, int nframes, int S, int ref_image, const int *included,
		int *shiftx, int *shifty, double *quality, bool normalize_q) {
	if (!ctx || ctx->dev.empty() || !sel || !shiftx || !shifty || !quality)
		return SG_ERR_GENERIC;
	if (nframes < 1 || S < 1)
		return SG_ERR_GENERIC;
	if (ref_image < 0)
		ref_image = 0;
	if (ref_image >= nframes)
		return set_err(ctx, SG_ERR_GENERIC, "reference image out of range%s %ld", "", ref_image);
	const size_t plane = (size_t)S * S;
	std::vector<int> todo;
	for (int f = 0; f < nframes; f++)
		if (f != ref_image && (!included || included[f]))
			todo.push_back(f);
	const int G = (int)std::max<size_t>(1, std::min(ctx->dev.size(), todo.size()));
	if (G == 1) {
		SgDevice &dv = ctx->dev[0];
		HIPCHK(hipSetDevice(dv.id));
		const size_t bytes = (size_t)nframes * plane * sizeof(uint16_t);
		HIPCHK(ensure(dv.reg_sel, bytes));
		HIPCHK(hipMemcpyAsync(dv.reg_sel.p, sel, bytes, hipMemcpyHostToDevice, dv.stream));
		return reg_dft_device(ctx, 0, (const uint16_t *)dv.reg_sel.p, (int64_t)S * S, S, nframes, S, ref_image, included,
				shiftx, shifty,
				quality, nullptr, normalize_q);
	}
	/* shard g: local frame 0 = the reference, 1..k = todo[t0 .. t1) */
	std::vector<int> rcs((size_t)G, SG_OK);
	std::vector<double> qraw((size_t)nframes, 0.0);
	std::vector<double> qref((size_t)G, 0.0);
	auto run = [&](int g) {
		const size_t t0 = todo.size() * (size_t)g / (size_t)G, t1 = todo.size() * (size_t)(g + 1) / (size_t)G;
		const int k = (int)(t1 - t0);
		SgDevice &dv = ctx->dev[(size_t)g];
		int &rc = rcs[(size_t)g];
		if (hipSetDevice(dv.id) != hipSuccess) {
			rc = set_err(ctx, SG_ERR_DEVICE, "hipSetDevice failed%s %ld", "", dv.id);
			return;
		}
		const size_t bytes = (size_t)(k + 1) * plane * sizeof(uint16_t);
		if (ensure(dv.reg_sel, bytes) != hipSuccess) {
			rc = set_err(ctx, SG_ERR_DEVICE, "no device memory for the selections%s (%ld frames)", "", k + 1);
			return;
		}
		uint16_t *d = (uint16_t *)dv.reg_sel.p;
		hipError_t e = hipMemcpyAsync(d, sel + (size_t)ref_image * plane, plane * sizeof(uint16_t),
				hipMemcpyHostToDevice, dv.stream);
		for (int j = 0; j < k && e == hipSuccess; j++)
			e = hipMemcpyAsync(d + (size_t)(j + 1) * plane, sel + (size_t)todo[t0 + (size_t)j] * plane,
					plane * sizeof(uint16_t), hipMemcpyHostToDevice, dv.stream);
		if (e != hipSuccess) {
			rc = set_err(ctx, SG_ERR_DEVICE, "selection upload failed%s %ld", "", g);
			return;
		}
		std::vector<int> lx((size_t)k + 1), ly((size_t)k + 1);
		std::vector<double> lq((size_t)k + 1);
		rc = reg_dft_device(ctx, g, d, (int64_t)S * S, S, k + 1, S, 0, nullptr, lx.data(), ly.data(), lq.data(), nullptr,
				false);
		if (rc)
			return;
		qref[(size_t)g] = lq[0];
		for (int j = 0; j < k; j++) {
			const int f = todo[t0 + (size_t)j];
			shiftx[f] = lx[(size_t)j + 1];
			shifty[f] = ly[(size_t)j + 1];
			qraw[(size_t)f] = lq[(size_t)j + 1];
		}
	};
	{
		/* a thread that cannot start fails its slot (and the call) instead of escaping the C ABI;
		 * the threads that did start are always joined */
		std::vector<std::thread> th;
		bool started = true;
		for (int g = 1; g < G; g++) {
			try {
				th.emplace_back(run, g);
			} catch (...) {
				for (int h = g; h < G; h++)
					rcs[(size_t)h] = set_err(ctx, SG_ERR_GENERIC, "could not start the thread of device slot%s %ld", "", h);
				started = false;
				break;
			}
		}
		if (started)
			run(0);
		else
			rcs[0] = SG_ERR_GENERIC;
		for (std::thread &t : th)
			t.join();
	}
	sg_stack_stats agg;
	memset(&agg, 0, sizeof agg);
	for (int g = 0; g < G; g++) {
		const sg_stack_stats &st = ctx->dev[(size_t)g].stats;
		agg.reg_ties_resolved += st.reg_ties_resolved;
		agg.reg_ties_unresolved += st.reg_ties_unresolved;
		agg.reg_fp64_reruns += st.reg_fp64_reruns;
		agg.reg_ms = std::max(agg.reg_ms, st.reg_ms);
	}
	{
		std::lock_guard<std::mutex> lk(ctx->mu);
		ctx->stats.reg_ties_resolved = agg.reg_ties_resolved;
		ctx->stats.reg_ties_unresolved = agg.reg_ties_unresolved;
		ctx->stats.reg_fp64_reruns = agg.reg_fp64_reruns;
		ctx->stats.reg_ms = agg.reg_ms;
	}
	for (int g = 0; g < G; g++)
		if (rcs[(size_t)g])
			return rcs[(size_t)g];
	shiftx[ref_image] = shifty[ref_image] = 0;
	quality[ref_image] = qref[0];
	for (int f : todo)
		quality[f] = qraw[(size_t)f];
	if (!normalize_q)
		return SG_OK;
	double q_min = qref[0], q_max = qref[0];
	for (int f : todo) {
		const double qv = qraw[(size_t)f];
		if (qv > q_max)
			q_max = qv;
		q_min = (q_min < qv) ? q_min : qv;
	}
	for (int f = 0; f < nframes; f++) {
		if (included && !included[f])
			continue;
		quality[f] -= q_min;
		quality[f] /= (q_max - q_min);
	}
	return SG_OK;
}

extern "C" int sg_register_dft_u16(sg_ctx *ctx, const uint16_t *sel, int nframes, int S, int ref_image,
		const int *included, int *shiftx, int *shifty, double *quality) {
	return reg_host(ctx, sel, nframes, S, ref_image, included, shiftx, shifty, quality, true);
}

extern "C" int sg_register_dft_u16_raw(sg_ctx *ctx, const uint16_t *sel, int nframes, int S, int ref_image,
		const int *included, int *shiftx, int *shifty, double *quality_raw) {
	return reg_host(ctx, sel, nframes, S, ref_image, included, shiftx, shifty, quality_raw, false);
}
