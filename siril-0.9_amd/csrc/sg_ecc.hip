/*
 * sg_ecc.hip - ECC registration of resident frames (include/sirilgpu.h, sg_register_ecc_u16*):
 * register_ecc (src/registration/registration.c:786-930) -> findTransform
 * (src/opencv/ecc/ecc.cpp:556-603) -> findTransform_ECC (:307-554) for WARP_MODE_TRANSLATION.
 * OpenCV is not pinned by the reference, so its published algorithm is restated (as in
 * sg_warp.hip); tests/ecc_ref.py is the literal numpy form the kernels are compared with.
 *
 *   k_ecc_prepare  convertTo(CV_8UC1) (saturating), GaussianBlur 5x5 sigma 0 ({1,4,6,4,1}/16
 *                  separable, BORDER_REFLECT_101).  For 8-bit input every partial sum is an
 *                  integer, so blurred * 256 <= 65280 is stored as u16: bit-faithful to the float
 *                  plane at 2 bytes a pixel.  Once for the reference frame (the template), once per
 *                  frame.
 *   k_ecc_iter     one loop body of findTransform_ECC for every unfinished frame of the chunk.  A
 *                  translation's fixed-point warp coordinates are one integer offset and one 1/32
 *                  fraction for the whole image (sge_offsets), so a workgroup's 64 x 32 output tile
 *                  reads one contiguous source tile with a 3-pixel halo, staged in LDS as floats.
 *                  The warped image and both warped gradients are formed per pixel with OpenCV's
 *                  float operations (sge_strip); the gradient planes are never stored.  The raw
 *                  moments (SGE_*) are summed in fp64 per thread, wave and workgroup, written as
 *                  per-workgroup partials, and the frame's last workgroup (an atomic ticket) adds
 *                  them in tile order and runs the scalar step (sg_ecc_step.h).  No
 *                  floating-point atomic, no wait of one workgroup on another: the result is the
 *                  same bits every run.  About 4 bytes of HBM traffic per pixel and iteration.
 *
 * The host enqueues the iteration launches back to back; a frame whose state says done costs its
 * workgroups one load each.  Every SGE_SYNC_EVERY launches the host reads the count of
 * unfinished frames and stops when it is 0.
 */
#include "sg_ctx.hpp"
#include "sg_ecc_plan.hpp"
#include <algorithm>
#include <vector>

struct SgEccPrepParams {
	const uint16_t *in;	/* frame f at in + f * frame_pitch, row r at + r * row_pitch */
	int64_t frame_pitch, row_pitch;
	uint16_t *out;		/* [nf][H][W] */
	const sge_state *st;	/* frames already done are skipped; NULL = all */
	int W, H;
};

static_assert(SGE_THREADS == 256 && SGE_TILE_W == 64, "a wave per strip row of the tile");

__global__ void __launch_bounds__(SGE_THREADS) k_ecc_prepare(SgEccPrepParams p) {
	__shared__ uint16_t s_in[SGE_IN_W * SGE_IN_H];
	__shared__ uint16_t s_mid[SGE_TILE_W * SGE_IN_H];
	const int f = blockIdx.z, tid = threadIdx.x;
	if (p.st && p.st[f].done)
		return;
	const int x0 = blockIdx.x * SGE_TILE_W, y0 = blockIdx.y * SGE_TILE_H;
	const uint16_t *img = p.in + (int64_t)f * p.frame_pitch;
	for (int idx = tid; idx < SGE_IN_W * SGE_IN_H; idx += SGE_THREADS)
		s_in[idx] = sge_prep_load(idx, img, p.row_pitch, p.W, p.H, x0, y0);
	__syncthreads();
	for (int idx = tid; idx < SGE_TILE_W * SGE_IN_H; idx += SGE_THREADS)
		s_mid[idx] = sge_prep_h(idx, s_in);
	__syncthreads();
	const int ox = tid % SGE_TILE_W, oy0 = (tid / SGE_TILE_W) * SGE_ROWS, x = x0 + ox;
	if (x >= p.W)
		return;
	uint16_t *out = p.out + (int64_t)f * p.W * p.H;
#pragma unroll
	for (int u = 0; u < SGE_ROWS; u++) {
		const int y = y0 + oy0 + u;
		if (y < p.H)
			out[(int64_t)y * p.W + x] = sge_prep_v(ox, oy0 + u, s_mid);
	}
}

struct SgEccIterParams {
	const uint16_t *planes;	/* [nf][H][W] blurred * 256 */
	const uint16_t *tmpl;	/* [H][W] */
	double *partial;	/* [nf][tiles][SGE_NMOM] */
	sge_state *st;		/* [nf] */
	unsigned int *ticket;	/* [nf], grows by `tiles` per iteration of an unfinished frame */
	int *nactive;		/* unfinished frames of the chunk */
	int W, H, tiles;
};

struct SgEccLds {
	float src[SGE_SRC_W * SGE_SRC_H];
	double red[SGE_THREADS / 64][SGE_NMOM];
	double tot[SGE_NMOM];
	int last;
};

/* the workgroup's sum of every moment, in a fixed order: lanes by shuffles, then wave 0 .. 3.
 * Returns moment `tid` to the threads tid < SGE_NMOM. */
__device__ static inline double sge_block_sum(const double *acc, SgEccLds &L, int tid) {
	const int lane = tid & 63, wave = tid >> 6;
#pragma unroll
	for (int m = 0; m < SGE_NMOM; m++) {
		double v = acc[m];
#pragma unroll
		for (int off = 32; off >= 1; off >>= 1)
			v += __shfl_down(v, off, 64);
		if (lane == 0)
			L.red[wave][m] = v;
	}
	__syncthreads();
	double t = 0.0;
	if (tid < SGE_NMOM)
		t = L.red[0][tid] + L.red[1][tid] + L.red[2][tid] + L.red[3][tid];
	return t;
}

__global__ void __launch_bounds__(SGE_THREADS) k_ecc_iter(SgEccIterParams p) {
	__shared__ SgEccLds L;
	const int f = blockIdx.z, tid = threadIdx.x;
	if (p.st[f].done)
		return;
	const SgeWarp w = sge_warp_setup(p.st[f].tx, p.st[f].ty);
	const int x0 = blockIdx.x * SGE_TILE_W, y0 = blockIdx.y * SGE_TILE_H;
	const int64_t npix = (int64_t)p.W * p.H;
	const uint16_t *plane = p.planes + (int64_t)f * npix;
	for (int idx = tid; idx < SGE_SRC_W * SGE_SRC_H; idx += SGE_THREADS)
		L.src[idx] = sge_src_load(idx, plane, p.W, p.H, x0 + w.iox - 1, y0 + w.ioy - 1);
	__syncthreads();
	double acc[SGE_NMOM];
#pragma unroll
	for (int m = 0; m < SGE_NMOM; m++)
		acc[m] = 0.0;
	sge_strip(tid, L.src, p.tmpl, p.W, p.H, x0, y0, w, acc);
	const double mine = sge_block_sum(acc, L, tid);
	const int tile = blockIdx.y * gridDim.x + blockIdx.x;
	double *part = p.partial + (int64_t)f * p.tiles * SGE_NMOM;
	if (tid < SGE_NMOM)
		part[(int64_t)tile * SGE_NMOM + tid] = mine;
	/* publish the partials, take a ticket; whoever draws the frame's last one this iteration reads
	 * them all behind an agent-scope acquire.  Nobody waits. */
	asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
	__syncthreads();
	if (tid == 0) {
		__builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
		asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
		const unsigned int t = __hip_atomic_fetch_add(&p.ticket[f], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
		L.last = (t + 1u) % (unsigned int)p.tiles == 0u;
		if (L.last) {
			__builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
			asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
		}
	}
	__syncthreads();
	if (!L.last)
		return;
#pragma unroll
	for (int m = 0; m < SGE_NMOM; m++)
		acc[m] = 0.0;
	for (int k = tid; k < p.tiles; k += SGE_THREADS) {
		const double *q = part + (int64_t)k * SGE_NMOM;
#pragma unroll
		for (int m = 0; m < SGE_NMOM; m++)
			acc[m] += q[m];
	}
	const double all = sge_block_sum(acc, L, tid);
	if (tid < SGE_NMOM)
		L.tot[tid] = all;
	__syncthreads();
	if (tid == 0) {
		sge_state s = p.st[f];
		sge_step(L.tot, &s);
		p.st[f] = s;
		if (s.done)
			atomicSub(p.nactive, 1);
	}
}

/* frame g's result goes to entry dest[g] of `out` (dest == NULL: entry g) */
static int sge_run(sg_ctx *ctx, int dev_index, const SgEccPlan &pl, const uint16_t *d_frames, const int *included,
		const int *dest, const sg_ecc_out *out, void *stream) {
	SgDevice &dv = ctx->dev[dev_index];
	HIPCHK(hipSetDevice(dv.id));
	hipStream_t s = sg_stream(dv, stream);
	const int W = pl.W, H = pl.H, chunk = pl.chunk;
	const size_t o_tmpl = 0, o_planes = o_tmpl + sg_up16(pl.plane_bytes);
	const size_t o_part = o_planes + sg_up16(pl.plane_bytes * chunk), o_st = o_part + sg_up16(pl.partial_bytes * chunk);
	const size_t o_tick = o_st + sg_up16(sizeof(sge_state) * chunk), o_act = o_tick + sg_up16(sizeof(unsigned int) * chunk);
	HIPCHK(ensure(dv.ecc_work, o_act + 16));
	char *wk = (char *)dv.ecc_work.p;
	SgEccPrepParams pp;
	pp.in = d_frames + (int64_t)pl.ref_image * pl.frame_pitch;
	pp.frame_pitch = pl.frame_pitch;
	pp.row_pitch = pl.row_pitch;
	pp.out = (uint16_t *)(wk + o_tmpl);
	pp.st = nullptr;
	pp.W = W;
	pp.H = H;
	hipLaunchKernelGGL(k_ecc_prepare, dim3((unsigned)pl.tiles_x, (unsigned)pl.tiles_y, 1u), dim3(SGE_THREADS), 0, s, pp);
	HIPCHK(hipGetLastError());
	SgEccIterParams ip;
	ip.planes = (const uint16_t *)(wk + o_planes);
	ip.tmpl = (const uint16_t *)(wk + o_tmpl);
	ip.partial = (double *)(wk + o_part);
	ip.st = (sge_state *)(wk + o_st);
	ip.ticket = (unsigned int *)(wk + o_tick);
	ip.nactive = (int *)(wk + o_act);
	ip.W = W;
	ip.H = H;
	ip.tiles = pl.tiles;
	std::vector<sge_state> hst(chunk);
	dv.ecc_prep_ms = dv.ecc_iter_ms = 0.;
	dv.ecc_launches = 0;
	for (int f0 = 0; f0 < pl.nframes; f0 += chunk) {
		const int nf = std::min(pl.nframes - f0, chunk);
		int nact = 0;
		for (int f = 0; f < nf; f++) {
			const int g = f0 + f;
			sge_state_init(&hst[f]);
			if (g == pl.ref_image || (included && !included[g]))
				hst[f].done = 1;
			else
				nact++;
		}
		if (nact > 0) {
			int hact = nact;
			HIPCHK(hipMemcpyAsync(ip.st, hst.data(), sizeof(sge_state) * nf, hipMemcpyHostToDevice, s));
			HIPCHK(hipMemcpyAsync(ip.nactive, &hact, sizeof(int), hipMemcpyHostToDevice, s));
			HIPCHK(hipMemsetAsync(ip.ticket, 0, sizeof(unsigned int) * nf, s));
			HIPCHK(hipStreamSynchronize(s));	/* the host copies above are read */
			const dim3 grid((unsigned)pl.tiles_x, (unsigned)pl.tiles_y, (unsigned)nf);
			pp.in = d_frames + (int64_t)f0 * pl.frame_pitch;
			pp.out = (uint16_t *)(wk + o_planes);
			pp.st = ip.st;
			HIPCHK(hipEventRecord(dv.ev[0], s));
			hipLaunchKernelGGL(k_ecc_prepare, grid, dim3(SGE_THREADS), 0, s, pp);
			HIPCHK(hipGetLastError());
			HIPCHK(hipEventRecord(dv.ev[1], s));
			for (int it = 0; it < SGE_MAX_ITER && hact > 0;) {
				for (int k = 0; k < SGE_SYNC_EVERY && it < SGE_MAX_ITER; k++, it++) {
					hipLaunchKernelGGL(k_ecc_iter, grid, dim3(SGE_THREADS), 0, s, ip);
					HIPCHK(hipGetLastError());
					dv.ecc_launches++;
				}
				HIPCHK(hipMemcpyAsync(&hact, ip.nactive, sizeof(int), hipMemcpyDeviceToHost, s));
				HIPCHK(hipStreamSynchronize(s));
			}
			float ms0 = 0.f, ms1 = 0.f;
			HIPCHK(hipEventRecord(dv.ev[2], s));
			HIPCHK(hipEventSynchronize(dv.ev[2]));
			HIPCHK(hipEventElapsedTime(&ms0, dv.ev[0], dv.ev[1]));
			HIPCHK(hipEventElapsedTime(&ms1, dv.ev[1], dv.ev[2]));
			dv.ecc_prep_ms += ms0;
			dv.ecc_iter_ms += ms1;	/* with the host's looks at the active count between the launches */
			if (hact != 0)
				return set_err(ctx, SG_ERR_GENERIC, "ecc: frames left unfinished after the last iteration%s: %ld", "", (long)hact);
			HIPCHK(hipMemcpyAsync(hst.data(), ip.st, sizeof(sge_state) * nf, hipMemcpyDeviceToHost, s));
			HIPCHK(hipStreamSynchronize(s));
		}
		for (int f = 0; f < nf; f++) {
			const int g = f0 + f;
			if (g != pl.ref_image && included && !included[g])
				continue;	/* neither registered nor written */
			sge_state r = hst[f];
			if (g == pl.ref_image) {	/* the reference frame: 0, 0 */
				sge_state_init(&r);
				r.rho = 1.0;
			}
			float dx, dy;
			int sx, sy;
			sge_result(&r, &dx, &dy, &sx, &sy);
			const int o = dest ? dest[g] : g;
			out->shiftx[o] = sx;
			out->shifty[o] = sy;
			if (out->dx)
				out->dx[o] = dx;
			if (out->dy)
				out->dy[o] = dy;
			if (out->rho)
				out->rho[o] = g == pl.ref_image ? 0.0 : r.rho;
			if (out->iterations)
				out->iterations[o] = r.iter;
			if (out->failed)
				out->failed[o] = r.failed;
		}
	}
	return SG_OK;
}

static int sge_check(sg_ctx *ctx, SgEccPlan &pl, const void *frames, int64_t frame_pitch, int64_t row_pitch, int W, int H,
		int nframes, int ref_image, const sg_ecc_out *out) {
	const int rc = sg_ecc_plan(W, H, nframes, ref_image, frame_pitch, row_pitch, 0, ctx->knobs.ecc_chunk, pl);
	if (rc != SG_OK)
		return set_err(ctx, rc, "%s", pl.err);
	if (!frames || !out || !out->shiftx || !out->shifty)
		return set_err(ctx, SG_ERR_GENERIC, "ecc: missing frames or shift arrays%s", "");
	return SG_OK;
}

extern "C" int sg_register_ecc_u16_device(sg_ctx *ctx, int dev_index, const uint16_t *d_frames, int64_t frame_pitch,
		int64_t row_pitch, int W, int H, int nframes, int ref_image, const int *included, const sg_ecc_out *out,
		void *stream) {
	if (!sg_dev_ok(ctx, dev_index))
		return SG_ERR_GENERIC;
	SgEccPlan pl;
	const int rc = sge_check(ctx, pl, d_frames, frame_pitch, row_pitch, W, H, nframes, ref_image, out);
	if (rc != SG_OK)
		return rc;
	return sge_run(ctx, dev_index, pl, d_frames, included, nullptr, out, stream);
}

/* host frames: the reference's layer and a batch of frames' layers are uploaded tight, slot 0 the
 * reference, and registered as a sequence of their own; a frame's result does not depend on its
 * neighbours, so this equals the device entry */
extern "C" int sg_register_ecc_u16(sg_ctx *ctx, const uint16_t *frames, int64_t frame_pitch, int64_t row_pitch, int W,
		int H, int nframes, int ref_image, const int *included, const sg_ecc_out *out) {
	if (!ctx || ctx->dev.empty())
		return SG_ERR_GENERIC;
	SgEccPlan pl;
	int rc = sge_check(ctx, pl, frames, frame_pitch, row_pitch, W, H, nframes, ref_image, out);
	if (rc != SG_OK)
		return rc;
	const size_t npix = (size_t)W * H;
	SgHostBatches hb(ctx);
	HIPCHK(hb.begin(nframes, npix, SG_HOST_BUDGET_1G, ctx->knobs.ecc_chunk, npix));
	HIPCHK(hb.upload_layer(hb.lead, frames + (int64_t)ref_image * pl.frame_pitch, W, H, pl.row_pitch));
	std::vector<int> inc(hb.batch + 1), dest(hb.batch + 1);
	inc[0] = 1;
	dest[0] = ref_image;	/* each batch writes the reference's own result again: the same values */
	while (hb.next()) {
		for (int f = 0; f < hb.nf; f++) {
			const int g = dest[1 + f] = hb.f0 + f;
			inc[1 + f] = g != ref_image && (!included || included[g]);
			HIPCHK(hb.upload_layer(hb.d + (size_t)f * npix, frames + (int64_t)g * pl.frame_pitch, W, H, pl.row_pitch));
		}
		SgEccPlan bp;
		rc = sg_ecc_plan(W, H, hb.nf + 1, 0, 0, 0, 0, ctx->knobs.ecc_chunk, bp);
		if (rc != SG_OK)
			return set_err(ctx, rc, "%s", bp.err);
		rc = sge_run(ctx, 0, bp, hb.lead, inc.data(), dest.data(), out, nullptr);
		if (rc != SG_OK)
			return rc;
	}
	return SG_OK;
}

extern "C" int sg_register_ecc_last_times(sg_ctx *ctx, int dev_index, double *prepare_ms, double *iterate_ms, int *launches) {
	if (!sg_dev_ok(ctx, dev_index))
		return SG_ERR_GENERIC;
	const SgDevice &dv = ctx->dev[dev_index];
	if (prepare_ms)
		*prepare_ms = dv.ecc_prep_ms;
	if (iterate_ms)
		*iterate_ms = dv.ecc_iter_ms;
	if (launches)
		*launches = dv.ecc_launches;
	return SG_OK;
}
