/*
 * sg_host_batch.hpp - the batch rule of the host-frame entries (sg_findstar, sg_findstar_fit,
 * sg_prepro_frames, sg_register_ecc_u16, sg_cosme_autodetect, sg_quality_u16), with no HIP in it, so
 * tests/test_host_batch_cpu.py builds it without a GPU.  SgHostBatches (sg_ctx.hpp) is the loop.
 */
#pragma once
#include <stddef.h>

/* u16 elements of host frames staged per batch */
#define SG_HOST_BUDGET_1G ((size_t)1 << 29)	/* 1 GiB: findstar, starfit, prepro, ECC */
#define SG_HOST_BUDGET_512M ((size_t)1 << 28)	/* 512 MiB: cosme, quality */

static inline size_t sg_up16(size_t v) {
	return (v + 15) & ~(size_t)15;
}

/* frames per host batch: as many of the `frames` as the budget takes, at least one, at most `cap`
 * when that is above 0 */
static inline size_t sg_host_batch_frames(size_t frames, size_t frame_elems, size_t budget, size_t cap) {
	const size_t fit = budget / frame_elems, m = fit < frames ? fit : frames, n = m < 1 ? 1 : m;
	return cap > 0 && cap < n ? cap : n;
}
