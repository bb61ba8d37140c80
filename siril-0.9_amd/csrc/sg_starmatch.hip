/*
 * sg_starmatch.hip - star matching of a whole sequence (include/sirilgpu.h, sg_starmatch):
 * new_star_match for every frame against the reference frame's list.
 *
 *   - k_starmatch: one workgroup of SGM_LANES threads per frame to match, one launch for the
 *     sequence.  The workgroup runs sg_starmatch.h's sgm_frame, the same chain of stages a host
 *     program runs with one lane, over a workspace in LDS (SgmWork; the layout and its byte count
 *     are stated there): both lists, the triangle arrays overlaid by the distances and the sums'
 *     partials, the vote matrices, the pairs and RANSAC's masks.  Votes and counts are integer LDS
 *     atomics; every floating-point sum has one fixed order, so a frame's bits do not depend on the
 *     run, on the other frames of the call or on the lane count.
 *   - The workspace is sized by the call's longest list: 162 KB at 2000 stars, one workgroup per
 *     CU (the work is a chain per frame and the frames fill the CUs), 80 KB at 60 stars.
 *   - Global memory holds only the packed (xpos, ypos, mag) triples, the table of frames, the
 *     results and the pairs.
 */
#include <hip/hip_runtime.h>
#include <string.h>
#include <vector>
#include "sg_ctx.hpp"
#include "sg_starmatch_plan.hpp"

static_assert(sizeof(sg_starmatch_result) == 256 && sizeof(SgStarmatchItem) == 16, "record layouts");
static_assert(sizeof(sg_star) == 112, "sg_star");

struct SgStarmatchParams {
	const double *packed;
	const SgStarmatchItem *items;
	sg_starmatch_result *res;	/* [grid] */
	int32_t *pairs;			/* [grid][MAX_STARS_FITTED][2] or NULL */
	int nmax;
};

__global__ void __launch_bounds__(SGM_LANES) k_starmatch(SgStarmatchParams p) {
	extern __shared__ __attribute__((aligned(16))) unsigned char s_mem[];
	const SgStarmatchItem it = p.items[blockIdx.x];
	const SgmWork w = sgm_work(s_mem, p.nmax);
	sgm_frame(w, (int)threadIdx.x, SGM_LANES, p.packed + it.a_off, p.packed, it.n, &p.res[blockIdx.x],
			p.pairs ? p.pairs + (size_t)blockIdx.x * 2 * MAX_STARS_FITTED : nullptr);
}

extern "C" int sg_starmatch(sg_ctx *ctx, int dev_index, int nframes, int max_stars, const int32_t *nstars, const sg_star *stars,
		int ref_image, const uint8_t *included, sg_starmatch_result *results, int32_t *pairs, void *stream) {
	if (!sg_dev_ok(ctx, dev_index))
		return SG_ERR_GENERIC;
	SgStarmatchPlan pl;
	const int rc = sg_starmatch_plan(nframes, max_stars, nstars, stars, ref_image, included, results, pairs != nullptr, pl);
	if (rc != SG_OK)
		return set_err(ctx, rc, "%s", pl.err);
	SgDevice &dv = ctx->dev[dev_index];
	dv.starmatch_ms = 0.;
	dv.starmatch_launches = 0;
	std::vector<sg_starmatch_result> got(pl.items.size());
	std::vector<int32_t> got_pairs;
	if (pl.grid) {
		HIPCHK(hipSetDevice(dv.id));
		hipStream_t s = sg_stream(dv, stream);
		HIPCHK(ensure(dv.starmatch_work, pl.packed_bytes + pl.table_bytes + pl.result_bytes + pl.pairs_bytes));
		char *wk = (char *)dv.starmatch_work.p;
		SgStarmatchParams q;
		q.packed = (const double *)wk;
		q.items = (const SgStarmatchItem *)(wk + pl.packed_bytes);
		q.res = (sg_starmatch_result *)(wk + pl.packed_bytes + pl.table_bytes);
		q.pairs = pairs ? (int32_t *)(wk + pl.packed_bytes + pl.table_bytes + pl.result_bytes) : nullptr;
		q.nmax = pl.nmax;
		HIPCHK(hipFuncSetAttribute((const void *)k_starmatch, hipFuncAttributeMaxDynamicSharedMemorySize, (int)pl.lds_bytes));
		HIPCHK(hipMemcpyAsync(wk, pl.packed.data(), pl.packed.size() * sizeof(double), hipMemcpyHostToDevice, s));
		HIPCHK(hipMemcpyAsync(wk + pl.packed_bytes, pl.items.data(), pl.items.size() * sizeof(SgStarmatchItem), hipMemcpyHostToDevice, s));
		HIPCHK(hipEventRecord(dv.ev[0], s));
		hipLaunchKernelGGL(k_starmatch, dim3(pl.grid), dim3(SGM_LANES), pl.lds_bytes, s, q);
		HIPCHK(hipGetLastError());
		HIPCHK(hipEventRecord(dv.ev[1], s));
		HIPCHK(hipMemcpyAsync(got.data(), q.res, got.size() * sizeof(sg_starmatch_result), hipMemcpyDeviceToHost, s));
		if (pairs) {
			got_pairs.resize(pl.items.size() * (size_t)2 * MAX_STARS_FITTED);
			HIPCHK(hipMemcpyAsync(got_pairs.data(), q.pairs, got_pairs.size() * sizeof(int32_t), hipMemcpyDeviceToHost, s));
		}
		HIPCHK(hipStreamSynchronize(s));
		float ms = 0.f;
		HIPCHK(hipEventElapsedTime(&ms, dv.ev[0], dv.ev[1]));
		dv.starmatch_ms = ms;
		dv.starmatch_launches = 1;
	}
	/* nothing of the caller's is written before the device work has succeeded */
	sgm_fill_unmatched(pl, max_stars, stars, results);
	const size_t per = (size_t)2 * MAX_STARS_FITTED;
	if (pairs)
		for (size_t i = 0; i < (size_t)nframes * per; i++)
			pairs[i] = -1;
	for (size_t b = 0; b < pl.items.size(); b++) {
		const SgStarmatchItem &it = pl.items[b];
		sg_starmatch_result &o = results[it.frame];
		o = got[b];
		if (o.status == SG_MATCH_OK)
			sgm_fwhm_average(stars + (size_t)it.frame * max_stars, it.n, &o.fwhmx, &o.fwhmy);
		if (pairs)
			memcpy(pairs + (size_t)it.frame * per, got_pairs.data() + b * per, per * sizeof(int32_t));
	}
	return SG_OK;
}

extern "C" int sg_starmatch_last_times(sg_ctx *ctx, int dev_index, double *ms, int *launches) {
	if (!sg_dev_ok(ctx, dev_index))
		return SG_ERR_GENERIC;
	const SgDevice &dv = ctx->dev[dev_index];
	if (ms)
		*ms = dv.starmatch_ms;
	if (launches)
		*launches = dv.starmatch_launches;
	return SG_OK;
}

extern "C" int sg_starmatch_warp_plan(const sg_starmatch_result *results, int nframes, double *hom, int *action, int *out_slot,
		int *new_total) {
	return sgm_warp_plan(results, nframes, hom, action, out_slot, new_total);
}
