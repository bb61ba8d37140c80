/*
 * sirilgpu.h - C ABI of libsirilgpu.so, the MI355X (gfx950) implementation of Siril 0.9's
 * sequence registration + stacking hot path.
 *
 * Plain C types only (no torch, no HIP types in signatures).  Each entry point cites the
 * reference interface whose body it replaces; the reference-side glue is shown in
 * INTEGRATION.md.
 *
 * Conventions:
 *   - WORD = uint16_t (src/core/siril.h:44).
 *   - Images are planar per channel and bottom-up ("memory order", src/core/siril.h:391-442).
 *   - A region read through sg_read_region_fn is a top-down band, exactly what
 *     seq_opened_read_region() returns (src/io/sequence.c:690-700).
 *   - Return codes mirror the reference: 0 ok, -1 generic/cancel/unsupported, -2 size or
 *     allocation error, -3 read failure (src/stacking/stacking.c:244-246,1212-1220).
 *   - Device work runs on the context's own non-blocking HIP stream (or the stream passed
 *     in): device buffers handed to a *_device call must be complete, i.e. the caller
 *     synchronises whatever produced them on other streams (a torch fill, a copy) first.
 */
#ifndef SIRILGPU_H
#define SIRILGPU_H

#include <stdint.h>
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SG_OK 0
#define SG_ERR_GENERIC -1
#define SG_ERR_SIZE -2
#define SG_ERR_READ -3
#define SG_ERR_DEVICE -10

/* stacking_methods[] order, src/stacking/stacking.c:54-56 */
enum sg_stack_method {
	SG_STACK_SUM = 0,	/* stack_summing            :196-355  */
	SG_STACK_MEAN = 1,	/* stack_mean_with_rejection :1189-1858 */
	SG_STACK_MEDIAN = 2,	/* stack_median             :362-816  */
	SG_STACK_MAX = 3,	/* stack_addmax             :824-972  */
	SG_STACK_MIN = 4	/* stack_addmin             :979-1128 */
};

/* src/stacking/stacking.h:14-21 */
enum sg_rejection { SG_NO_REJEC, SG_PERCENTILE, SG_SIGMA, SG_SIGMEDIAN, SG_WINSORIZED, SG_LINEARFIT };
/* src/stacking/stacking.h:24-30 */
enum sg_normalization { SG_NO_NORM, SG_ADDITIVE, SG_MULTIPLICATIVE, SG_ADDITIVE_SCALING,
	SG_MULTIPLICATIVE_SCALING };

/* kernel selection for sg_stack_desc.kernel_path (results are identical on every path) */
enum sg_kernel_path { SG_PATH_AUTO = 0, SG_PATH_SORTED = 1 };

/* rectangle, src/core/siril.h:477-479 */
typedef struct { int x, y, w, h; } sg_rect;

/* shape of seq_opened_read_region (src/io/sequence.h:17): fill `buffer` with the top-down
 * band `area` of channel `layer` of frame `index`; <0 on failure */
typedef int (*sg_read_region_fn)(void *user, int layer, int index, uint16_t *buffer,
		const sg_rect *area);
/* get_thread_run() (src/core/processing.c:294-300): 0 = cancel requested */
typedef int (*sg_should_continue_fn)(void *user);

/* What a stack_method needs from struct stacking_args + sequence (src/stacking/stacking.h:38-56,
 * src/core/siril.h:328-374), flattened to plain arrays.  Per-frame arrays are indexed by the
 * stacked-frame position i (the reference's image_indices[i] order). */
typedef struct {
	int method;		/* enum sg_stack_method */
	int rejection;		/* enum sg_rejection (SG_STACK_MEAN only) */
	int normalize;		/* enum sg_normalization (MEAN and MEDIAN) */
	double sig[2];		/* args->sig */
	int nb_frames;		/* args->nb_images_to_stack */
	int width, height, nb_layers;	/* seq->rx, seq->ry, naxes[2] */
	const int *shiftx;	/* regparam[reglayer][image_indices[i]].shiftx, or NULL */
	const int *shifty;	/* ... .shifty, or NULL (no registration data) */
	const double *offset;	/* normalisation coefficients (compute_normalization), or NULL */
	const double *mul;
	const double *scale;
	int max_thread;		/* com.max_thread: the reference's OpenMP team size */
	int max_number_of_rows;	/* args->max_number_of_rows */
	int kernel_path;	/* SG_PATH_*: 0 = automatic (no reference equivalent; testing/A-B) */
	/* memory rows [resident_rows[0], resident_rows[1]) of every frame are present at
	 * d_frames (sg_stack_u16_device); {0, 0} = all rows [0, height).  No reference
	 * equivalent: it lets a rank hold only its row band plus the rows its shifts reach. */
	int resident_rows[2];
	int flags;		/* SG_STACK_* flags below (0 = none) */
	int reserved[2];
} sg_stack_desc;
/* sg_stack_desc.flags: the output is needed only once sg_stack_collect has returned, so an
 * async call (sg_stack_u16_device_async) may run its work after the main kernel (redo lists,
 * replay, counters) beside the next call's main kernel instead of on `stream`.  That work still
 * READS d_frames and WRITES d_out after `stream` has moved on: both must stay unchanged (the
 * frames) and unread (the output) until sg_stack_collect returns, or until work queued on a
 * stream after sg_stack_wait_tail(ctx, dev, stream) */
#define SG_STACK_RESULT_AT_COLLECT 1

typedef struct sg_ctx sg_ctx;

/* Open the devices this context drives: devs[0..ndev) (NULL: 0..ndev-1), ndev = 0 device 0,
 * ndev < 0 every visible device.  An id may repeat (context slots sharing one card).  One HIP
 * stream per slot; the host-pull calls (sg_stack_u16, sg_register_dft_u16) drive every slot
 * from its own host thread. */
int sg_init(sg_ctx **ctx, int ndev, const int *devs);
void sg_shutdown(sg_ctx *ctx);
const char *sg_last_error(const sg_ctx *ctx);

/*
 * Host-pull stack: replaces the bodies of stack_summing / stack_mean_with_rejection /
 * stack_median / stack_addmax / stack_addmin (src/stacking/stacking.c:196,1189,362,824,979).
 * Every device of the context takes a contiguous share of the output rows (the reference's
 * row blocks, :1397-1476, are the natural shard) and is driven by its own host thread, whose
 * readers (the reference's team size max_thread shared between the devices, at most 8 per
 * device) pull that share's frame rows through `pull` (seq_opened_read_region shape, called
 * concurrently as the reference's OpenMP team does) into pinned staging and upload them
 * directly to that device; a share larger than the device's HBM budget is stacked in row bands.
 * The result is written bottom-up into `out` (nb_layers*H*W WORDs, the buffer the reference
 * hands to gfit.data).  rej receives the per-channel low/high rejection counters of
 * :1796-1817 (MEAN only, summed over the devices), maxim the sum maximum of :311-313 (SUM only,
 * over the whole image; the 65535/max scaling uses it on every device).  `cont` is polled once
 * per frame read (get_thread_run, :1539); a cancellation returns SG_ERR_GENERIC.
 */
int sg_stack_u16(sg_ctx *ctx, const sg_stack_desc *desc, sg_read_region_fn pull, void *user,
		sg_should_continue_fn cont, void *cont_user, uint16_t *out, uint64_t rej[3][2],
		uint64_t *maxim);

/*
 * Device-resident stack (frames already in HBM).  d_frames holds frame i, channel c, memory
 * row r, column x at d_frames[i*frame_stride + c*plane_stride + r*width + x].  Output rows
 * [row_begin, row_end) (memory order) of every channel are written to d_out (same indexing
 * as a [C][H][W] image).  `stream` is a hipStream_t (NULL = the context's stream of device
 * `dev_index`).  The call is synchronous.
 *
 * Row bands (one rank per band): the band's output rows read frame rows
 * [row_begin - max(shifty), row_end - min(shifty)) (clipped to the frame), and those rows
 * must lie inside desc->resident_rows (else SG_ERR_SIZE); a rank holding only them may pass a
 * base pointer biased by -resident_rows[0]*width.  A rejection stack whose FIRST sigma pass
 * breaks early (`N - r <= 4`, stacking.c:1684) reads the previous pixel's stale rejected[]
 * (SURVEY §8a a3 iii); the previous pixel in the reference's OpenMP thread order can lie
 * outside the band, and is then recomputed from the frames.  If its rows are not resident
 * the call fails with SG_ERR_GENERIC instead of guessing: for such stacks (in practice
 * small N with strong rejection) make the full frames resident.
 *
 * Refused regime (both entry points): a MEAN stack (stack_mean_with_rejection, any rejection;
 * stack_median ignores shifts) whose shifts make a row block
 * of the reference's partition (max_thread, max_number_of_rows; :1397-1476) with start_row > 0
 * read above the frame.  The reference then writes offset = W*(area.y - shifty) past its block
 * buffer (stacking.c:1555-1561, a heap overflow with an undefined result); the call fails with
 * SG_ERR_GENERIC and a message instead of zero-filling.  Keep |shifty| below the block height.
 * Second refused regime: a SIGMEDIAN pixel whose clipping loop (stacking.c:1696-1709, no pass
 * cap) never ends, i.e. a pass replaces samples by the values they already hold (e.g. {0, 0,
 * 1, 1} with sig[1] < 0.87) or the pixel needs more than 4096 passes; Siril hangs there, the
 * call fails with SG_ERR_GENERIC.
 */
int sg_stack_u16_device(sg_ctx *ctx, int dev_index, const sg_stack_desc *desc,
		const uint16_t *d_frames, int64_t frame_stride, int64_t plane_stride,
		uint16_t *d_out, int row_begin, int row_end, uint64_t rej[3][2], uint64_t *maxim,
		void *stream);
/*
 * The same stack queued without waiting for it (replaces the same loop body as
 * sg_stack_u16_device, for callers that keep several stacks in flight, e.g. a row band per call
 * in a loop: the host prepares the next call while the device works).  Every launch decision is
 * made on the device, so nothing here waits for the GPU except reusing a counter slot: at most
 * two calls per device slot are pending, a third folds the oldest.  Successive async calls of a
 * device slot must use one stream.  sg_stack_collect waits for every pending call of the slot
 * and returns the SUM of their rejection counters, the maximum of their SUM maxima and the first
 * error any of them met (SG_ERR_GENERIC for the refused regimes above); statistics then describe
 * the last folded call.
 */
int sg_stack_u16_device_async(sg_ctx *ctx, int dev_index, const sg_stack_desc *desc,
		const uint16_t *d_frames, int64_t frame_stride, int64_t plane_stride,
		uint16_t *d_out, int row_begin, int row_end, void *stream);
int sg_stack_collect(sg_ctx *ctx, int dev_index, uint64_t rej[3][2], uint64_t *maxim);
/* device-side ordering for SG_STACK_RESULT_AT_COLLECT calls (no reference equivalent: the
 * reference's blocks are synchronous): work queued on `stream` (NULL = the slot's own stream)
 * after this returns waits for every tail kernel the slot's async calls have queued so far, so
 * a band loop may refill d_frames, or read / send d_out, on its stream without a host wait */
int sg_stack_wait_tail(sg_ctx *ctx, int dev_index, void *stream);

/* Statistics of the last stack call on this context (for bench.py / rocprof cross-checks). */
typedef struct {
	double kernel_ms;	/* HIP-event time of the main stacking kernel(s) on their stream */
	double total_ms;	/* HIP-event time of the whole device-side stack call */
	uint64_t slow_pixels;	/* pixels re-done by the literal (fp80) path */
	uint64_t chain_pixels;	/* pixels needing the cross-pixel stale-state replay */
	uint64_t launches;	/* kernels launched by the main path */
	int main_kernel_blocks;
	int path;		/* main path of a MEAN stack: 1 = histogram (k_stack_hist), 0 = other */
	/* last registration: frames whose correlation maximum was a near tie, decided by exact
	 * integer correlations / left to the FFT arg-max (more candidates than the cap) */
	uint64_t reg_ties_resolved, reg_ties_unresolved;
	uint64_t reg_fp64_reruns;	/* pairs of the fp32 passes re-run in fp64 (near ties at fp32 tolerance) */
	uint64_t compact_pixels;	/* normalised histogram stacks: redo pixels whose sorted columns the
					 * histogram kernel wrote out (no gather in the sorted kernel) */
	double reg_ms;			/* last registration on a device: HIP-event span of its device work
					 * (first pass to the quality estimate's end, host waits included) */
	int64_t norm_fma;		/* normalised histogram stack: the sample load found equal to the reference's roundings
					 * for every u16 value of every frame: 2 = an integer offset (additive, scale 1), 1 = one
					 * fma per sample; 0 = the reference's operations */
} sg_stack_stats;
int sg_get_last_stats(const sg_ctx *ctx, sg_stack_stats *st);
/* device slots of the context (sg_init's ndev): callers size their batches by it, as the
 * reference sizes its work by com.max_thread (src/core/siril.h:596) */
int sg_device_count(const sg_ctx *ctx, int *ndev);

/*
 * Per-frame normalisation statistics: location / scale of layer 0 as
 * statistics(fit, 0, NULL, STATS_IKSS, STATS_ZERO_NULLCHECK) computes them
 * (src/algos/statistics.c:152-326; the imstats _compute_normalization_for_image reads,
 * src/stacking/stacking.c:79-123).  d_frames: nframes frames [C][H][W] in Siril memory order
 * at frame_stride elements (0 = C*H*W); location / scale: host arrays [nframes].
 * 0, or SG_ERR_GENERIC when a frame has no non-zero pixel (statistics() returns NULL).
 */
int sg_frame_stats_ikss_device(sg_ctx *ctx, int dev_index, const uint16_t *d_frames, int nframes, int C,
		int H, int W, int64_t frame_stride, double *location, double *scale, void *stream);
/* the same on host frames (what seq_get_imstats computes from a loaded frame) */
int sg_frame_stats_ikss(sg_ctx *ctx, const uint16_t *frames, int nframes, int C, int H, int W,
		double *location, double *scale);
/* compute_normalization (src/stacking/stacking.c:125-190): offset / mul / scale [nframes]
 * from per-frame location / scale (host arithmetic; ref_image -1 = 0) */
int sg_compute_normalization(int mode, int nframes, int ref_image, const double *location,
		const double *scale_in, double *offset, double *mul, double *scale);

/*
 * DFT registration: replaces register_shift_dft (src/registration/registration.c:182-400).
 * d_sel / sel hold nframes bottom-up S x S selections (what seq_read_frame_part returns,
 * src/io/sequence.c:567-609), any side 4 <= S <= 4096 (FFTW plans every size, :251-257).
 * included may be NULL (process_all_frames).  Outputs the integer shifts and the normalised
 * quality (normalizeQualityData :163-176) per frame.  A correlation maximum whose runner-up
 * lies within the FFT tolerance is decided by exact integer correlations (sg_stack_stats
 * reg_ties_*).
 */
int sg_register_dft_u16(sg_ctx *ctx, const uint16_t *sel, int nframes, int S, int ref_image,
		const int *included, int *shiftx, int *shifty, double *quality);
/* the same with the qualities left RAW (QualityEstimate of the reference and of every
 * registered frame): the glue replays the reference's q_min / q_max / q_index bookkeeping and
 * normalizeQualityData itself, which a cancelled registration skips (registration.c:166-168).
 * Host selections: with several devices in the context the frames are split into contiguous
 * shards, one host thread per device. */
int sg_register_dft_u16_raw(sg_ctx *ctx, const uint16_t *sel, int nframes, int S, int ref_image,
		const int *included, int *shiftx, int *shifty, double *quality_raw);
int sg_register_dft_u16_device(sg_ctx *ctx, int dev_index, const uint16_t *d_sel, int nframes,
		int S, int ref_image, const int *included, int *shiftx, int *shifty,
		double *quality, void *stream);
/*
 * The same on a shard of the sequence's frames (frame sharding over GPUs):
 * quality is left RAW (QualityEstimate per registered frame and the reference,
 * src/algos/quality.c:46-218; NaN where no pixel passes the threshold), so the caller can
 * gather every shard's values and apply normalizeQualityData (registration.c:163-176) with
 * the reference's min/max loop over all frames (sirilgpu_dist.register_sharded).  Frames
 * outside `included` are neither registered nor written.
 */
int sg_register_dft_u16_device_raw(sg_ctx *ctx, int dev_index, const uint16_t *d_sel, int nframes,
		int S, int ref_image, const int *included, int *shiftx, int *shifty,
		double *quality_raw, void *stream);

/*
 * The same on selections read IN PLACE from resident frames (no extraction copy): selection f,
 * bottom-up row r, column x at d_sel[f * frame_pitch + r * row_pitch + x] (elements; row_pitch >=
 * S), e.g. a window of layer `layer` of [C][H][W] frames: d_sel = frames + layer H W + y0 W + x0,
 * frame_pitch = C H W, row_pitch = W.  What seq_read_frame_part (src/io/sequence.c:567-609)
 * extracts per frame is thus read by the first pass itself.  raw_quality != 0: the quality is
 * left raw as in sg_register_dft_u16_device_raw.
 */
int sg_register_dft_u16_device_pitched(sg_ctx *ctx, int dev_index, const uint16_t *d_sel, int64_t frame_pitch,
		int64_t row_pitch, int nframes, int S, int ref_image, const int *included, int *shiftx, int *shifty,
		double *quality, int raw_quality, void *stream);

/*
 * Perspective warp: replaces cvTransformImage (src/opencv/opencv.cpp:242-309) as the
 * star-alignment registration uses it (src/registration/registration.c:719-723, flip /
 * warp / flip): memory-order (bottom-up) planes in, memory-order planes out of size
 * out_width x out_height (ref.x, ref.y); hom = Homography h00..h22 row-major (the
 * forward map, inverted as warpPerspective does without WARP_INVERSE_MAP);
 * interpolation = opencv_interpolation (src/core/siril.h:257-264: 0 nearest, 1 linear,
 * 2 area (= linear), 3 cubic, 4 lanczos4), border constant 0.  OpenCV's algorithm is
 * restated (sg_warp.hip); OpenCV is unpinned, so parity is unpinned.
 */
int sg_warp_u16(sg_ctx *ctx, const uint16_t *in, int width, int height, int nb_layers,
		uint16_t *out, int out_width, int out_height, const double *hom, int interpolation);
int sg_warp_u16_device(sg_ctx *ctx, int dev_index, const uint16_t *d_in, int width, int height,
		int nb_layers, uint16_t *d_out, int out_width, int out_height, const double *hom,
		int interpolation, void *stream);

/*
 * The same warp on a whole resident sequence, one homography per frame: the loop body of
 * register_star_alignment after the matching (src/registration/registration.c:655-755), which
 * warps every layer of every frame and writes the compacted r_ sequence.  Frame f of the source is
 * nb_layers planes of width x height at d_in + f * frame_pitch elements (0 = tight); hom holds
 * nframes x 9 doubles (h00..h22 per frame, host memory).  action[f] (host, NULL = all APPLY):
 *   SG_WARP_SKIP   the frame is excluded, has too few stars or its match failed: nothing is written;
 *   SG_WARP_APPLY  the frame is warped;
 *   SG_WARP_COPY   the reference frame, saved unwarped (:678); needs equal source and output sizes.
 * out_slot[f] (host, NULL = f) is the output frame the result goes to, the reference's
 * frame - failed - skipped, at d_out + out_slot[f] * out_frame_pitch elements.  Every byte of a
 * written frame equals what sg_warp_u16_device gives for that frame and homography (a singular
 * homography is a zero matrix there too).
 * Refused before any device work, with a message for sg_last_error: SG_ERR_SIZE for a dimension
 * <= 0, a plane of 2^31 pixels or more, nb_layers outside 1..3, nframes < 1, a pitch below one
 * frame; SG_ERR_GENERIC for a missing pointer, an interpolation outside 0..4, an unknown action, COPY
 * with unequal sizes, a slot below 0 on a written frame, two written frames with one slot, and
 * source and output byte ranges that overlap.
 * With a stream the device entry returns once its work is queued on it.  sg_warp_frames_u16 takes
 * host sequences (the pitches then apply to them), staged in batches of at most 1 GiB of source
 * frames (SG_HOST_BATCH caps the frames per batch).
 * sg_warp_frames_last_times waits for the last call on that device and gives its device span, its
 * kernel launches, the destination tiles that took their taps from LDS and from global memory, and
 * the pixels of LDS tiles whose window lay outside the staged box and were read from global memory
 * (0 unless the footprint bound of csrc/sg_warp_tile.h is wrong: speed, never the result, depends
 * on it).  By default linear and Lanczos-4 take the LDS route, nearest and cubic read global memory
 * (the measured faster way of each).  Environment knob, read at sg_init: SG_WARP_ROUTE=1 sends every
 * tile to global memory, 2 every tile whose box fits to LDS, whatever the interpolation.
 */
typedef struct sg_warp_seq_desc {
	int width, height, nb_layers;		/* source frames: planar, memory order (bottom-up), 1..3 layers */
	int out_width, out_height;		/* ref.x, ref.y */
	int interpolation;			/* opencv_interpolation 0..4, 2 (area) = linear, as sg_warp_u16 */
	int64_t frame_pitch, out_frame_pitch;	/* elements between frames, 0 = tight */
} sg_warp_seq_desc;

enum { SG_WARP_SKIP = 0, SG_WARP_APPLY = 1, SG_WARP_COPY = 2 };

int sg_warp_frames_u16_device(sg_ctx *ctx, int dev_index, const sg_warp_seq_desc *desc, const uint16_t *d_in, int nframes,
		const double *hom, const int *action, const int *out_slot, uint16_t *d_out, void *stream);
int sg_warp_frames_u16(sg_ctx *ctx, const sg_warp_seq_desc *desc, const uint16_t *in, int nframes, const double *hom,
		const int *action, const int *out_slot, uint16_t *out);
int sg_warp_frames_last_times(sg_ctx *ctx, int dev_index, double *ms, int *launches, uint64_t *tiles_lds,
		uint64_t *tiles_gather, uint64_t *pixels_stray);

/*
 * Sequence preprocessing: replaces the loop body of seqpreprocess (src/core/siril.c:1019-1169):
 * darkOptimization (:963-985), preprocess (:945-961: imoper SUB :150-187, fdiv :252-275) and
 * cosmeticCorrection (src/algos/cosmetic_correction.c:275-294), on frames resident in HBM, in
 * place.  Everything is exact integer / fp64 arithmetic written as the reference writes it, so
 * the calibrated frames and the fitted dark scale equal the reference's bit for bit.
 *
 * Masters are host [C][H][W] memory-order images with the frames' nb_layers (the reference does
 * not check this and reads absent planes); NULL = that master is not used (USE_OFFSET / USE_DARK /
 * USE_FLAT of com.preprostatus).  They are taken as 16-bit images: an 8-bit master (whose
 * statistics use a 256-bin histogram) is out of scope.
 *   - `normalisation` is a float, as in struct preprocessing_data (src/core/siril.h:306-313);
 *     autolevel sets it to (float) of the mean of the non-zero pixels of the flat's layer 0
 *     (statistics() -> FnMeanSigma_ushort, src/algos/quantize.c:126-190).  A flat without a
 *     non-zero pixel makes the reference give up: SG_ERR_GENERIC.
 *   - dark_optimization (USE_OPTD): per frame a golden-section search of k in [0, 2] (13
 *     iterations, goldenSectionSearch :922-943) minimising the background noise (the noise1 slot
 *     of fits_img_stats_ushort, FnNoise1_ushort quantize.c:658-783, null value 0) of
 *     max(raw - round_to_WORD(dark * k), 0) on layer 0.  A row whose sigma-clipped differences
 *     give a negative variance (sum2 / n - mean * mean < 0: a NaN row) makes the reference's
 *     qsort order undefined; such frames are unpinned.
 *   - cosmetic (USE_COSME): the hot / cold pixels of the master dark (find_deviant_pixels
 *     :176-240) are repaired in every frame, in the reference's list order, in place.  It applies
 *     only to one-layer sequences; otherwise the reference logs and skips it, and so does this
 *     (sg_prepro_info.cosmetic_applies = 0).  The dark's median is read from the reference's
 *     histogram, whose 65536 bins cover [0, 65535): pixels of value 65535 fall outside and are not
 *     counted, while they still count in the number of good pixels (src/gui/histogram.c:111-127).
 *     PARITY-UNPINNED READ: for a cold pixel with all 24 neighbours inside the frame,
 *     getMedian5x5 (:34-67) reads value[-1], one element before its heap block (undefined).  It
 *     is taken as 0 here: that is what the n < 24 cases read by construction (a padding zero of
 *     the calloc'ed array) and what glibc's chunk header holds in practice.  A deviant pixel
 *     without any neighbour in the frame (a 1-pixel-wide or -high image) divides 0 by 0 in the
 *     reference; it is set to 0 here.
 * Refused with SG_ERR_GENERIC, nothing substituted: dark optimization with nb_layers != 1 (the
 * reference extracts layer 0 into a one-layer image and then indexes layers 1 and 2 of it), dark
 * optimization without a dark, cosmetic without a dark.  SG_ERR_SIZE: a dimension <= 0, or a
 * plane of 2^31 pixels or more.
 */
typedef struct {
	int width, height, nb_layers;
	const uint16_t *offset, *dark, *flat;	/* host [C][H][W], or NULL */
	int dark_optimization;	/* USE_OPTD */
	int cosmetic;		/* USE_COSME */
	double cosme_sigma[2];	/* args->sigma: {cold, hot}, -1 = that side off */
	int is_cfa;		/* args->is_cfa: same-colour neighbours (step 2) */
	int autolevel;		/* args->autolevel */
	float normalisation;	/* args->normalisation (used when autolevel == 0) */
} sg_prepro_desc;

typedef struct {
	double level;			/* the float level used by the flat division, as a double */
	int64_t icold, ihot;		/* deviant pixels of the master dark */
	double thres_cold, thres_hot;
	double dark_sigma, dark_median;
	int cosmetic_applies;		/* 0: not requested, or skipped (nb_layers != 1) */
	/* schedule of the in-place correction: connected components of "lies in the other's
	 * window", each walked in list order by one lane */
	int64_t components, longest_component;
} sg_prepro_info;

typedef struct sg_prepro sg_prepro;

/* all per-sequence work, once: derived masters uploaded to device `dev_index`, the level, the
 * deviant list and its schedule */
int sg_prepro_create(sg_ctx *ctx, int dev_index, const sg_prepro_desc *desc, sg_prepro **out);
void sg_prepro_free(sg_prepro *pp);
int sg_prepro_get_info(const sg_prepro *pp, sg_prepro_info *info);
/* calibrate nframes resident frames in place: frame f, channel c, row r at
 * d_frames[f*frame_stride + (c*height + r)*width] (frame_stride 0 = C*H*W; the layout of
 * sg_frame_stats_ikss_device).  dark_k[nframes] (may be NULL) receives the fitted k of each frame
 * ("Dark optimization: %.3lf"), 1.0 without dark optimization.  Synchronous. */
int sg_prepro_frames_device(sg_ctx *ctx, int dev_index, sg_prepro *pp, uint16_t *d_frames, int nframes,
		int64_t frame_stride, double *dark_k, void *stream);
/* the same on host frames [nframes][C][H][W] (upload, run, download) on device 0 of the context
 * (the prepro object must have been created there) */
int sg_prepro_frames(sg_ctx *ctx, sg_prepro *pp, uint16_t *frames, int nframes, double *dark_k);
/* the search's objective alone: noise[f] = evaluateNoiseOfCalibratedImage (:886-918) of frame f
 * at k[f], i.e. the reference's bgnoise of max(raw - round_to_WORD(dark * k), 0) on layer 0; the
 * frames are not changed.  Needs a dark. */
int sg_prepro_noise_device(sg_ctx *ctx, int dev_index, sg_prepro *pp, const uint16_t *d_frames, int nframes,
		int64_t frame_stride, const double *k, double *noise, void *stream);

/*
 * Star candidates: the whole-image part of peaker (src/algos/star_finder.c:103-255), which
 * register_star_alignment calls once per frame (src/registration/registration.c:583-586, :682),
 * on frames resident in HBM.  Integer, fp32 and fp64 arithmetic in the reference's order, so the
 * records, the detection plane, the candidate list and the boxes equal the reference's bit for bit.
 *   1. Threshold (Compute_threshold :39-57): statistics(fit, layer, NULL, STATS_BASIC,
 *      STATS_ZERO_NULLCHECK): ngood = the non-zero pixels, sigma from FnMeanSigma_ushort's
 *      sequential double sums, median from computeHisto's 65536 bins over [0, 65535) (65535 is not
 *      binned but counts in ngood; from bin 1, the first bin whose running count exceeds
 *      ngood * 0.5, else 0).  threshold = (WORD)((WORD)median + sigma_k * (WORD)sigma), norm =
 *      65535, bg = median.
 *   2. Detection plane (get_wavelet_layers(.., 3, 2, TO_PAVE_BSPLINE, layer),
 *      src/core/siril.c:1285-1336): pave_2d_bspline_smooth with Step 1, then Step 2
 *      (src/algos/pave.c:227-284) of (float)image, indices clamped, operand order kept, quantised
 *      by reget_rawdata (src/algos/reconstr.c:120-140).
 *   3. Peak test (:176-199) in display (top-down) coordinates over y in [aY0 + r, aY1 - r),
 *      x in [aX0 + r, aX1 - r): p > threshold, p < norm, no greater 8-neighbour, no equal
 *      neighbour in the row above or to the left.  Candidates in raster order (y outer, x inner).
 *   4. Boxes (:203-211): the 2r x 2r pixels of the ORIGINAL image around a candidate in gsl_matrix
 *      order, boxes[ii * 2r + jj] = top[y - r + jj][x - r + ii], as uint16_t.
 * Kept quirks, each reported per frame:
 *   - min(width, height) < 32: wavelet_transform_data refuses (src/algos/transform.c:194-201),
 *     peaker ignores it, and the detection plane is the unsmoothed image (wavelet_applied = 0);
 *   - a frame without a non-zero pixel: statistics() returns NULL and the reference goes on with an
 *     uninitialised norm and bg; here such a frame has no candidate (no_data = 1), the call succeeds;
 *   - PARITY-UNPINNED: a threshold of 65536 or more is undefined in C; the x86-64 result (truncated
 *     to int32, low 16 bits) is taken and threshold_wrapped = 1;
 *   - reget_rawdata rescales a plane whose float maximum exceeds 65535 (ratio_applied = 1; no
 *     input reaches it);
 *   - sigma_on_host = 1: the frame's sum of squares reached 2^53, where the reference's double
 *     sums round, and the plane was summed sequentially on the host.
 * Refused before any device work: SG_ERR_SIZE for a dimension <= 0, a plane of 2^31 pixels or
 * more, layer outside [0, nb_layers), an area not inside the image (the reference reads out of
 * bounds); SG_ERR_GENERIC for radius < 1 (the 3x3 test would leave the image), sigma negative or
 * not finite, max_candidates < 0.  2 * radius >= a side of the area is no error: no candidate.
 * Left to the caller: the PSF fit (psf_global_minimisation(z, bg = median, layer, FALSE, FALSE),
 * GSL, unpinned) with xpos = x + x0 - r - 1, ypos = y + y0 - r - 1 (:221-222), is_star, the
 * MAX_STARS cap on accepted stars (the reference has no cap on candidates) and sort_stars, which
 * sg_findstar_fit* does; the matching (new_star_match) is sg_starmatch, below; see INTEGRATION.md.
 */
typedef struct {
	int width, height, nb_layers;
	int layer;
	int radius;		/* sf->radius */
	double sigma;		/* sf->sigma, the k of the threshold */
	int use_area;
	sg_rect area;		/* display (top-down) coordinates, used when use_area != 0 */
	int max_candidates;	/* capacity of cand_xy / boxes per frame */
} sg_findstar_desc;

typedef struct {
	int64_t ngood;
	double median, sigma;
	int threshold;
	int64_t ncand;		/* candidates found */
	int64_t nstored;	/* min(ncand, max_candidates): the first ones in raster order */
	int wavelet_applied, ratio_applied, sigma_on_host, threshold_wrapped, no_data;
} sg_findstar_frame;

/* frames: frame f, channel c, row r at d_frames[f*frame_stride + (c*height + r)*width]
 * (frame_stride 0 = C*H*W; the layout of sg_prepro_frames_device); never written.
 * per_frame[nframes]; cand_xy: host [nframes][max_candidates][2] int32, (x, y) in display
 * coordinates; boxes: host [nframes][max_candidates][2r * 2r] uint16, may be NULL; d_wave: device
 * [nframes][H][W], memory order, receives the detection plane, may be NULL.  Synchronous. */
int sg_findstar_device(sg_ctx *ctx, int dev_index, const sg_findstar_desc *desc, const uint16_t *d_frames,
		int nframes, int64_t frame_stride, sg_findstar_frame *per_frame, int32_t *cand_xy, uint16_t *boxes,
		uint16_t *d_wave, void *stream);
/* the same on host frames [nframes][C][H][W] on device 0 of the context; wave: host
 * [nframes][H][W], may be NULL */
int sg_findstar(sg_ctx *ctx, const sg_findstar_desc *desc, const uint16_t *frames, int nframes,
		sg_findstar_frame *per_frame, int32_t *cand_xy, uint16_t *boxes, uint16_t *wave);

/*
 * Fitted stars: all of peaker (src/algos/star_finder.c:103-255) for resident frames.  After the
 * candidates of sg_findstar*, each stored candidate's 2r x 2r box is fitted on the device
 * (psf_global_minimisation(z, bg = median, layer, FALSE, FALSE), src/algos/PSF.c:46-157, 160-220,
 * 314-428, 620-662): the start values of psf_init_data bit for bit, then GSL's lmsder on
 * psf_Gaussian_f / _df restated in fp64 (siril-0.9_amd/csrc/sg_psf.h, DESIGN.md §6: PARITY-UNPINNED
 * against any one GSL build, checked against tests/psf_ref.py within a measured tolerance), the
 * finish, psf_update_units as the two factors fwhm_scale_x / _y, is_star, xpos = x + x0 - r - 1 and
 * ypos = y + y0 - r - 1.  The boxes never leave the device.  Per frame the accepted stars are the
 * first max_stars in raster (candidate) order, returned sorted ascending by mag, ties by cand (the
 * reference's qsort leaves ties open and its OpenMP order depends on timing; the serial order is
 * the contract).  Kept quirks: the box is transposed (matrix rows run along image x, x0 belongs to
 * image y) and xpos / ypos are taken literally; a half-maximum walk that does not move gives S = 0,
 * a fit that is not finite, SG_FIT_NONFINITE.  Departures: rmse is taken at the final x (the
 * reference reports the solver's last model evaluation, which may be a refused trial step); the
 * relative uncertainties are not computed (the reference does not use them).
 * Refused before any device work, beyond what sg_findstar refuses: SG_ERR_GENERIC for radius > 32,
 * roundness or a scale not finite, norm not 255 or 65535, max_stars outside [0, 50000].
 * radius = 1 is no error: every candidate gets SG_FIT_NOT_ENOUGH_PIXELS.
 * The matching (new_star_match) and FWHM_average take these lists as they are: sg_starmatch, below.
 * Left to the caller: the angle fit, the uncertainties, 8-bit frames.
 */
#define SG_STARFIT_MAX_RADIUS 32
#define SG_STARFIT_MAX_STARS 50000	/* MAX_STARS */

enum {
	SG_FIT_STAR = 0,
	SG_FIT_NOT_ENOUGH_PIXELS = 1,	/* n <= 6 */
	SG_FIT_NONFINITE = 2,
	SG_FIT_BAD_FWHM = 3,		/* FWHM not finite or <= 0 */
	SG_FIT_NOT_STAR = 4,		/* is_star refused it: failed_test says where */
	SG_FIT_OVER_CAP = 5		/* a star beyond the first max_stars */
};

typedef struct {
	sg_findstar_desc find;
	double roundness;	/* sf->roundness */
	double norm;		/* get_normalized_value(&gfit): 255 or 65535, of the DISPLAYED image */
	double fwhm_scale_x, fwhm_scale_y;	/* psf_update_units' factors; 1.0 while the units stay pixels */
	int max_stars;		/* capacity of stars per frame, at most SG_STARFIT_MAX_STARS */
	int want_candidates;	/* fill cands */
} sg_starfit_desc;

/* an accepted star; B, A and rmse are normalised, sx >= sy, fwhm in the scaled units */
typedef struct {
	int32_t cand;		/* index in the frame's candidate list */
	int32_t x, y;		/* the candidate, display coordinates */
	int32_t iters;		/* outer iterations of the solver */
	double B, A, x0, y0, sx, sy, fwhmx, fwhmy, mag, rmse, xpos, ypos;
} sg_star;

/* every stored candidate, for diagnosis */
typedef struct {
	int32_t x, y;
	int32_t iters;
	int32_t status;		/* SG_FIT_* */
	int32_t failed_test;	/* SG_FIT_NOT_STAR: 1 .. 8, the test of is_star (:60-75) that failed */
	int32_t reserved;
	double init[6];		/* the start values B, A, x0, y0, SX, SY */
	double B, A, x0, y0, sx, sy, fwhmx, fwhmy, mag, rmse, xpos, ypos;
} sg_starfit_cand;

/* frames as in sg_findstar_device.  per_frame[nframes]; nstars: host [nframes] int32; stars: host
 * [nframes][max_stars], the first nstars[f] of frame f written; cands: host
 * [nframes][find.max_candidates], the first nstored written, NULL unless want_candidates.
 * Synchronous. */
int sg_findstar_fit_device(sg_ctx *ctx, int dev_index, const sg_starfit_desc *desc, const uint16_t *d_frames,
		int nframes, int64_t frame_stride, sg_findstar_frame *per_frame, int32_t *nstars, sg_star *stars,
		sg_starfit_cand *cands, void *stream);
/* the same on host frames [nframes][C][H][W] on device 0 of the context */
int sg_findstar_fit(sg_ctx *ctx, const sg_starfit_desc *desc, const uint16_t *frames, int nframes,
		sg_findstar_frame *per_frame, int32_t *nstars, sg_star *stars, sg_starfit_cand *cands);

/*
 * ECC registration: replaces the loop body of register_ecc (src/registration/registration.c:786-930),
 * findTransform (src/opencv/ecc/ecc.cpp:556-603) with WARP_MODE_TRANSLATION, 50 iterations, eps
 * 0.001, on frames resident in HBM.  OpenCV is not pinned by the reference: its published algorithm
 * is restated (tests/ecc_ref.py is the literal form), so parity is unpinned, as for sg_warp_u16.
 * Per frame != ref_image, in memory-order coordinates:
 *   - convertTo(CV_8UC1) SATURATES (min(v, 255), no rescale: the method is meant for 8-bit data held
 *     in WORDs), GaussianBlur 5x5 sigma 0, reflect-101; gradients (-0.5, 0, 0.5);
 *   - up to 50 iterations of: warp image and gradients by the current translation (warpAffine's
 *     1/32-pixel fixed point, bilinear, border 0; nearest for the mask), masked means and norms,
 *     2x2 Hessian, rho, lambda, the update of (tx, ty); it ends when |rho - last_rho| < 0.001;
 *   - success when rho > 0: dx = tx, dy = ty; -1 < rho <= 0 is success with dx = dy = 0 (findTransform
 *     returns (int)rho and the caller's memset zeros stand); rho = -1 or a non-finite rho or update:
 *     failed, the frame is to be excluded (incl = FALSE) and its shifts are 0;
 *   - shiftx = -round_to_int(dx), shifty = -round_to_int(dy).
 * The reference frame gets shifts 0, dx = dy = 0, rho 0, iterations 0, failed 0.  Frames outside
 * `included` (NULL = all) are neither registered nor written.  The quality register_ecc also stores
 * (QualityEstimate of the whole layer) is sg_quality_u16_device's, below; see INTEGRATION.md.
 * Frames are read in place: frame f, row r, column x at d_frames[f * frame_pitch + r * row_pitch + x]
 * (elements; 0 = tight: row_pitch W, frame_pitch H * row_pitch), e.g. layer `layer` of [C][H][W]
 * frames: d_frames = frames + layer H W, frame_pitch = C H W, row_pitch = W; never written.
 * SG_ERR_SIZE with a message: W or H below 8 or above 65536, a plane of 2^31 pixels or more,
 * nframes < 1, row_pitch < W, frame_pitch below a frame's extent, ref_image outside [0, nframes).
 * Synchronous; results are the same bits on every run.
 */
typedef struct {
	int *shiftx, *shifty;	/* host [nframes] */
	float *dx, *dy;		/* host [nframes], may be NULL */
	double *rho;		/* host [nframes], may be NULL: the last correlation coefficient */
	int *iterations;	/* host [nframes], may be NULL: loop bodies run */
	int *failed;		/* host [nframes], may be NULL: 1 = findTransform failed */
} sg_ecc_out;
int sg_register_ecc_u16_device(sg_ctx *ctx, int dev_index, const uint16_t *d_frames, int64_t frame_pitch,
		int64_t row_pitch, int W, int H, int nframes, int ref_image, const int *included, const sg_ecc_out *out,
		void *stream);
/* the same on host frames with the same pitches, uploaded in batches, on device 0 of the context */
int sg_register_ecc_u16(sg_ctx *ctx, const uint16_t *frames, int64_t frame_pitch, int64_t row_pitch, int W, int H,
		int nframes, int ref_image, const int *included, const sg_ecc_out *out);

/* the last ECC call on that device: the device time of its per-frame prepare launches, of its
 * iteration launches (HIP events; the second span includes the host's reads of the unfinished-frame
 * count between groups of launches) and the number of iteration launches.  Any pointer may be NULL. */
int sg_register_ecc_last_times(sg_ctx *ctx, int dev_index, double *prepare_ms, double *iterate_ms, int *launches);

/*
 * Automatic cosmetic correction: seqfind_cosme / seqfind_cosme_cfa / find_cosme and the GUI's
 * "Cosmetic Correction" (apply_cosmetic_to_sequence -> cosmetic_image_hook -> autoDetect,
 * src/algos/cosmetic_correction.c:296-435; process_findcosme, src/core/command.c:1294-1318) on
 * frames resident in HBM, in place, bit for bit.  Per frame and per layer 0 .. nb_layers - 1 in
 * turn, on the plane in memory order (y outer, x inner):
 *   1. statistics(fit, layer, NULL, STATS_BASIC | STATS_AVGDEV, STATS_ZERO_NULLCHECK): ngood = the
 *      non-zero pixels; bkg = the histogram median over bins 1 .. 65534 (the first bin whose running
 *      count exceeds ngood * 0.5, else 0; 65535 is not binned but counts in ngood); avgDev = the sum
 *      of |v - bkg| over the non-zero pixels (an exact integer) divided by ngood in double.
 *      ngood == 0: autoDetect returns 1, the frame fails at this layer (status = 1, failed_layer),
 *      the earlier layers stay corrected, this and the later ones are untouched.  A failed frame
 *      does not fail the call.
 *   2. the scan: a = getAverage3x3, m = getMedian5x5 (step 2, radius 2 / 4 with is_cfa; the
 *      start = 24 - n - 1 quirk: the median of one zero and the n - 1 smallest in-frame neighbours),
 *      both of the buffer as it stands when the scan reaches the pixel, so a pixel sees the
 *      corrections of the pixels before it.  Hot, unless sig[1] == -1:
 *      a < bkg + avgDev / 2 && pixel > bkg + avgDev && pixel > m + sig[1] * avgDev: ihot++,
 *      buf = a * amount + pixel * (1 - amount), in double as written, truncated to WORD.  Cold,
 *      unless sig[0] == -1: pixel + avgDev * sig[0] < bkg && pixel + avgDev * sig[0] < m: icold++,
 *      buf = m * amount + pixel * (1 - amount).
 *   3. icold and ihot are summed over the layers of a frame.
 * The result is the serial scan's for every input and the same bits on every run.  A pixel without
 * any neighbour at distance `step` (only CFA planes of at most 3 x 3 have one) takes a = 0 where
 * the reference converts a NaN.
 * Refused before any device work: SG_ERR_SIZE for a dimension <= 0, a plane of 2^31 pixels or
 * more, nb_layers outside [1, 3], nframes < 1, a frame_stride below one frame, a plane in which no
 * pixel has a neighbour (width <= step and height <= step: the reference divides 0 by 0);
 * SG_ERR_GENERIC for a sig that is NaN or negative and not exactly -1, an amount outside [0, 1].
 * amount is a parameter: process_findcosme leaves it uninitialised, the GUI sets it.
 * Left to the caller: writing the cc_ sequence, the list-driven `cosme` command, sharding over
 * devices; see INTEGRATION.md.
 */
typedef struct {
	int width, height, nb_layers;
	double sig[2];		/* {cold, hot}; -1 switches the test off */
	double amount;
	int is_cfa;
} sg_cosme_desc;

typedef struct {
	int status;		/* 0: corrected; 1: a layer without a non-zero pixel */
	int failed_layer;	/* that layer, else -1 */
	int64_t icold, ihot;
	double bkg[3], avg_dev[3];	/* per layer reached (0 for the others) */
} sg_cosme_frame;

/* frames: frame f, channel c, row r at d_frames[f*frame_stride + (c*height + r)*width]
 * (frame_stride 0 = C*H*W), corrected in place; out[nframes].  nframes = 1 is find_cosme.
 * Synchronous. */
int sg_cosme_autodetect_device(sg_ctx *ctx, int dev_index, const sg_cosme_desc *desc, uint16_t *d_frames,
		int nframes, int64_t frame_stride, void *stream, sg_cosme_frame *out);
/* the same on host frames [nframes][C][H][W], in place, uploaded in batches, on device 0 of the
 * context */
int sg_cosme_autodetect(sg_ctx *ctx, const sg_cosme_desc *desc, uint16_t *frames, int nframes,
		sg_cosme_frame *out);
/* the last call on that device: device time (HIP events) of its statistics, main pass and
 * dependence resolution (with the host's looks at the active count), the rounds launched, and the
 * pixels re-examined by them.  Any pointer may be NULL. */
int sg_cosme_last_times(sg_ctx *ctx, int dev_index, double *stat_ms, double *main_ms, double *resolve_ms,
		int *rounds, int64_t *reexamined);

/*
 * Quality of whole layers: QualityEstimate(fit, layer, QUALTYPE_NORMAL) (src/algos/quality.c:46-218),
 * the number register_ecc stores per frame (src/registration/registration.c:833, 892), of W x H planes
 * resident in HBM, bit for bit with oracle/or_registration.c: or_quality_estimate and the same bits
 * on every run.  Only subsample 3 contributes (quality.c:192-194 weights the others by an integer
 * quotient that is 0).  On the plane in memory order, as fit->pdata[layer] is:
 *   1. xs = (W - 1) / 3, ys = (H - 1) / 3; with xs < 2 || ys < 2 the result is 0.0, nothing is launched;
 *   2. sample (j, i) = the integer average of rows 3j .. 3j + 2, columns 3i .. 3i + 2;
 *   3. max = the largest sample of rows 1 .. ys - 2 with 0 < v < 65530;
 *   4. max > 0: v = (unsigned)((double)v * (60000.0 / max)) clamped at 65535, in fp64 as written;
 *   5. the 3 x 3 integer box / 9, the border ring 0;
 *   6. xb = (int)(xs * 0.1) + 1, yb = (int)(ys * 0.1) + 1: a pixel inside the margins whose smoothed
 *      value is >= 10240 flags its 3 x 3 neighbourhood; flagged pixels inside the margins add
 *      d1^2 + d2^2 (differences to the right and to the next row) and count;
 *   7. sqrt(val / pixels / 10), NaN when nothing passed the threshold.
 * The sums are exact integers, converted once: equality with the reference's double accumulation
 * holds while val < 2^53 (the limit the DFT path's quality has too).
 * Frames are read in place: frame f, row r, column x at d_frames[f * frame_pitch + r * row_pitch + x]
 * (elements; 0 = tight: row_pitch W, frame_pitch H * row_pitch), e.g. layer `layer` of [C][H][W]
 * frames: d_frames = frames + layer H W, frame_pitch = C H W, row_pitch = W; never written.  Any
 * base alignment, odd widths and odd pitches are taken.
 * quality_raw: host [nframes]; frames outside `included` (NULL = all) are not written.
 * A frame small enough for one workgroup's LDS (up to 40952 samples, e.g. 640 x 480) is estimated by
 * one workgroup without scratch; larger planes go through a u16 sample plane in HBM, in chunks of
 * frames.  Both routes give the same bits.
 * SG_ERR_SIZE with a message, before any device work: W or H <= 0, a plane of 2^31 pixels or more,
 * nframes < 1, row_pitch < W, frame_pitch below a frame's extent.  Synchronous.
 * Left to the caller: sharding a sequence over devices.  The DFT path (sg_register_dft_*) keeps its
 * own quality of the square selection.
 */
int sg_quality_u16_device(sg_ctx *ctx, int dev_index, const uint16_t *d_frames, int64_t frame_pitch, int64_t row_pitch,
		int W, int H, int nframes, const int *included, double *quality_raw, void *stream);
/* the same on host frames with the same pitches, uploaded in batches, on device 0 of the context */
int sg_quality_u16(sg_ctx *ctx, const uint16_t *frames, int64_t frame_pitch, int64_t row_pitch, int W, int H,
		int nframes, const int *included, double *quality_raw);
/* the last quality call on that device: the device time of its launches (HIP events), the route
 * taken (0: none, xs < 2 || ys < 2; 1: resident, one workgroup per frame; 2: tiled) and the number
 * of kernel launches.  Any pointer may be NULL. */
int sg_quality_last_times(sg_ctx *ctx, int dev_index, double *ms, int *route, int *launches);

/*
 * The bookkeeping of register_ecc around the raw values (registration.c:838, 899-905) and
 * normalizeQualityData (:163-176).  No context is needed.
 *   q_min = q_max = quality_raw[ref_image], q_index = ref_image; then for frame = 0 .. nframes - 1,
 *   frame != ref_image, measured[frame] (NULL = all), in index order:
 *       if (qual > q_max) { q_max = qual; q_index = frame; }   q_min = q_min < qual ? q_min : qual;
 *   so a NaN behaves as it does there (it never raises q_max; it replaces q_min, and the next
 *   measured value replaces it again).  The serial order is the contract.
 *   quality[frame] = quality_raw[frame] for the reference and the measured frames, 0 for the others
 *   (ECC leaves out the frames whose findTransform failed; their regdata stays zeroed); then every
 *   frame with normalized[frame] (NULL = all) becomes (quality - q_min) / (q_max - q_min), by a
 *   subtraction and a division as written (q_max == q_min divides by 0 as the reference does).
 * quality may be quality_raw.  q_min, q_max, q_index, msg may be NULL.  SG_ERR_SIZE: nframes < 1 or
 * ref_image outside [0, nframes); SG_ERR_GENERIC: a missing array; the reason goes to msg.
 */
int sg_quality_normalize(int nframes, int ref_image, const double *quality_raw, const int *measured,
		const int *normalized, double *quality, double *q_min, double *q_max, int *q_index, char *msg, int msg_len);

/*
 * "Stack the best percent % of the frames": compute_highest_accepted_quality
 * (src/stacking/stacking.c:2283-2310), stack_filter_quality (:2204-2213) and
 * fill_list_of_unfiltered_images (:2230-2241).  quality[i] is the value of every frame, included or
 * not (included NULL = all).  If an included frame has a negative quality: *threshold = 0.0,
 * *nselected = 0, SG_OK (the reference logs and returns 0.0).  Otherwise the values are sorted
 * ascending, *threshold = val[(int)((100.0 - percent) * (double)nframes / 100.0)], and selected[]
 * (host [nframes], may be NULL for the count alone) receives, in index order, the frames with
 * included && quality > 0.0 && quality >= threshold.  SG_ERR_GENERIC with the reason in msg where the
 * reference reads outside its array (an index >= nframes or < 0, e.g. percent 0) and where a value is
 * NaN (its sort is then undefined).  No context is needed.
 */
int sg_quality_select(int nframes, const double *quality, const int *included, double percent, double *threshold,
		int *selected, int *nselected, char *msg, int msg_len);

/*
 * One-star registration: seqpsf (src/io/sequence.c:1627-1820) and register_shift_fwhm
 * (src/registration/registration.c:406-490) on frames resident in HBM: the PSF of one star in a
 * rectangular selection of every frame, and the shifts that align the star.  Per processed frame
 * (frames outside `included` get SG_SEQPSF_EXCLUDED and nothing else), with the area (x, y, w, h) in
 * display (top-down) coordinates and W x H frames bottom-up in memory:
 *   1. the area: the call's; REGISTERED first applies x -= shiftx[f], y += shifty[f]
 *      (core/processing.c:85-137); FOLLOW_STAR starts from the carried area of step 6.  Then
 *      enforce_area_in_image (sequence.c:1123-1130) on a local copy: x < 0 -> 0, y < 0 -> 0,
 *      x + w > W -> W - w, y + h > H -> H - h.
 *   2. the box z[i][j] = memory row H - y - h + i, column x + j; i < h rows, j < w columns
 *      (PSF.c:583-608).  Not transposed, unlike peaker's box.
 *   3. bg = background() (core/siril.c:1173-1192): the median of statistics(STATS_BASIC,
 *      STATS_ZERO_NULLCHECK) (statistics.c:47-63, 207-256; histogram.c:129-150): ngood = the non-zero
 *      pixels, 65536 bins over [0, 65535) (65535 is not binned but counts in ngood), from bin 1 the
 *      first bin whose running count exceeds ngood * 0.5, else 0; ngood = 0 gives bg = 0.0 and the
 *      fit goes on.
 *   4. psf_minimiz_no_angle (PSF.c:46-157, 314-428): psf_init_data on the h x w box (getMedian3x3
 *      with its zero padding and its 8 - n - 1 offset, the first maximum in row-major order, the
 *      half-maximum walks bounded by NbRows - 1 / NbCols - 1), x_init = {bg, max, (jj1 + jj2 + 2) / 2,
 *      (ii1 + ii2 + 2) / 2, (size_t)(SQR(jj1 - jj2) / 4 / ln 2), (size_t)(SQR(ii1 - ii2) / 4 / ln 2)},
 *      lmsder on psf_Gaussian_f / _df as siril-0.9_amd/csrc/sg_psf.h restates it; n = w h <= 6: no PSF.
 *   5. psf_minimiz_angle (PSF.c:229-309, 434-559) when |SX - SY| >= 0.01 on the result of 4: lmsder
 *      with p = 7 on psf_Gaussian_f_an / _df_an literally (columns 2 and 3 keep cos(alpha), column 6
 *      as written), from {B, A, x0, y0, SX, SY, 0}, at most 10 iterations, test_delta(1e-4, 1e-4);
 *      angle = -alpha 180 / pi folded by `while (fabs(angle) > 90) angle -+= 90`; mag =
 *      -2.5 log10(sum(z - B)); fwhm = sqrt(S / 2) 2 sqrt(2 ln 2); rmse at the final x (the departure
 *      sg_findstar_fit documents).
 *   6. psf_global_minimisation (PSF.c:620-662): sy > sx swaps sx / sy and fwhmx / fwhmy, and a fitted
 *      angle != 0 gets -= 90 when positive, else += 90; B, A, rmse divided by norm; no PSF when a FWHM
 *      is not finite or <= 0; psf_update_units as the two factors; xpos = x0 + area.x, ypos = area.y +
 *      area.h - y0 with the clamped area of 1.  FOLLOW_STAR: the carried (unclamped) area becomes
 *      x = round_to_int(xpos) - w / 2, y = round_to_int(ypos) - h / 2 (integer division;
 *      core/utils.c:60-66).
 *   7. a frame with no PSF makes the reference abort the sequence and store nothing; here its status
 *      says so, and in FOLLOW_STAR the frames after it are not run (SG_SEQPSF_NOT_RUN).
 * Departure: the angle fold is bounded; a fold of more than 8 steps reports SG_FIT_NONFINITE.
 * ORIGINAL and REGISTERED run one workgroup per frame; FOLLOW_STAR is one launch of one workgroup
 * that walks the included frames in index order with no host look between them.
 * Frames are read in place with the pitches of sg_register_ecc_u16_device and never written.
 * Refused before any device work: SG_ERR_SIZE for w or h < 1 or > SG_SEQPSF_MAX_SIDE, w > W, h > H,
 * nframes < 1, and the pitch and size conditions sg_register_ecc_u16_device refuses; SG_ERR_GENERIC
 * for an unknown framing, REGISTERED without shifts, norm != 65535, a scale that is not finite, a
 * missing pointer.  w h <= 6 is no error: every frame gets SG_FIT_NOT_ENOUGH_PIXELS (and stops a
 * FOLLOW_STAR chain at its first frame).
 * Left to the caller: photometry (for_photometry = TRUE), the relative uncertainties, 8-bit
 * statistics, date_obs and exposure bookkeeping, areas above 128 pixels a side, sharding over devices.
 */
enum { SG_SEQPSF_ORIGINAL = 0, SG_SEQPSF_REGISTERED = 1, SG_SEQPSF_FOLLOW_STAR = 2 };
#define SG_SEQPSF_MAX_SIDE 128     /* w, h <= 128: the box (<= 16384 px, 32 KiB as u16) lives in LDS */
/* statuses: the SG_FIT_* values 0..3 keep their meaning (0 = a PSF), plus */
enum { SG_SEQPSF_NOT_RUN = 6,      /* FOLLOW_STAR: a frame after the one that stopped the chain */
       SG_SEQPSF_EXCLUDED = 7 };

typedef struct {
	int framing;               /* SG_SEQPSF_* */
	sg_rect area;              /* display coordinates; need not lie inside the image (step 1) */
	double norm;               /* 65535 (255 refused: 8-bit statistics are out of scope) */
	double fwhm_scale_x, fwhm_scale_y;
	int fit_angle;             /* 1 = seqpsf; 0 stops after step 4 (diagnosis, and the tests' way to pin step 4 alone) */
} sg_seqpsf_desc;

typedef struct {
	int32_t status, angle_fitted, iters, iters_angle;
	int32_t area_x, area_y;    /* the clamped area the box was read from */
	int64_t ngood;
	double bg, init[6], noangle[6];   /* start values; x after the 6-parameter fit */
	double B, A, x0, y0, sx, sy, fwhmx, fwhmy, angle, mag, rmse, xpos, ypos;
} sg_seqpsf_frame;

/* frame f, row r, column x at d_frames[f * frame_pitch + r * row_pitch + x] (elements; 0 = tight).
 * included: host [nframes], NULL = all.  reg_shiftx / reg_shifty: host [nframes], required for
 * REGISTERED only.  per_frame: host [nframes].  area_carry may be NULL; when non-NULL and FOLLOW_STAR
 * it replaces desc->area's x and y as the chain's starting (unclamped) area on entry, and on return
 * holds the carried area after the last frame run ({x, y} of desc->area in the other framings).
 * SG_OK even when frames have no PSF: the statuses say so.  Synchronous; the same bits on every run. */
int sg_seqpsf_u16_device(sg_ctx *ctx, int dev_index, const sg_seqpsf_desc *desc, const uint16_t *d_frames,
		int64_t frame_pitch, int64_t row_pitch, int W, int H, int nframes, const int *included, const int *reg_shiftx,
		const int *reg_shifty, sg_seqpsf_frame *per_frame, sg_rect *area_carry, void *stream);
/* the same on host frames with the same pitches, uploaded in batches, on device 0 of the context; a
 * FOLLOW_STAR chain is carried from batch to batch, so every batch size gives the same bits, and the
 * frames of the batches after a stopped chain are marked without being uploaded */
int sg_seqpsf_u16(sg_ctx *ctx, const sg_seqpsf_desc *desc, const uint16_t *frames, int64_t frame_pitch, int64_t row_pitch,
		int W, int H, int nframes, const int *included, const int *reg_shiftx, const int *reg_shifty,
		sg_seqpsf_frame *per_frame, sg_rect *area_carry);
/* the last seqpsf call on that device: device time (HIP events) and kernel launches; after the host
 * entry, the sums over its batches.  Either pointer may be NULL. */
int sg_seqpsf_last_times(sg_ctx *ctx, int dev_index, double *ms, int *launches);
/* register_shift_fwhm's second step from the records, host only, no context.  ref_image < 0 means 0.
 * Returns 1 when a frame that is not excluded has a status other than 0 (seqpsf aborted; outputs
 * untouched), -1 when the reference frame is excluded (outputs untouched), else 0 with: shifts 0 for
 * the reference and the excluded frames, else shiftx = round_to_int(ref.xpos - xpos), shifty =
 * round_to_int(ypos - ref.ypos); fwhm[f] = fwhmx (0 for excluded frames); the best frame by the loop
 * as written: it starts at the reference's fwhmx and is replaced when fwhm[f] < fwhm_min && fwhm[f] >
 * 0, scanning in frame order without revisiting the reference.  fwhm, best_index, best_fwhm may be NULL. */
int sg_seqpsf_shifts(int nframes, int ref_image, const sg_seqpsf_frame *per_frame, int *shiftx, int *shifty, double *fwhm,
		int *best_index, double *best_fwhm);

/*
 * Star matching of a whole sequence: the middle of register_star_alignment's loop
 * (src/registration/registration.c:589-755), new_star_match (src/registration/matching/match.c:125-389)
 * for every frame against the reference frame's list, one workgroup per frame in one launch.  With it
 * the chain is sg_findstar_fit* -> sg_starmatch -> sg_starmatch_warp_plan -> sg_warp_frames_u16*.
 * nstars [nframes] and stars [nframes][max_stars] are what sg_findstar_fit* returns (host arrays, each
 * list ascending by mag); the call packs (xpos, ypos, mag) and uploads it.  fitted_stars = min(nstars[ref],
 * 2000); frame f is matched with nbpoints = min(nstars[f], fitted_stars) stars of both lists.
 * Per frame, as the reference: atFindTrans (linear order, 20 brightest, triangle radius 0.002, scale
 * limits 0.9 .. 1.1, and once more without the scale test if that fails: scale_retry), atApplyTrans,
 * atMatchLists (radius 5), atCalcRMS (sx, sy), atRecalcTrans over the matched pairs, and cvCalculH:
 * findHomography with RANSAC (threshold 3, confidence 0.995, at most 2000 iterations, OpenCV's
 * generator seeded afresh), runKernel on the inliers and refine (at most 10 iterations).
 * siril-0.9_amd/csrc/sg_starmatch.h is the restatement, tests/starmatch_ref.py its literal numpy form
 * and the place of the contracts: ties of the reference's qsorts go to the smaller index; the matched
 * pairs are per A star the nearest candidate (ties to the smaller (x, id) of B), then per B star the
 * nearest A (ties to the smaller A id), in ascending B id; fewer than 6 winners of 2 votes is a failure
 * (the reference reads past them).  PARITY-UNPINNED: cvEigenVV and cvSVD are OpenCV internals, restated
 * as one cyclic Jacobi eigen-solver, as for the warp and ECC.
 * results [nframes]; status: SG_MATCH_REFERENCE (nbpoints = fitted_stars, hom = identity), EXCLUDED,
 * FEW_STARS (nstars[f] < 10), NO_TRANS (atFindTrans failed twice), NO_RECALC, NO_HOMOGRAPHY, or OK with
 * hom = h00 .. h22 as sg_warp_frames_u16* takes it.  nwinners = trans->nr of atFindTrans, trans0 its
 * TRANS (a .. f), trans / nr_recalc / sig those of atRecalcTrans; fwhmx / fwhmy = FWHM_average over the
 * first nbpoints stars (OK and REFERENCE frames); shiftx = +h02, shifty = -h12 (translation_only).
 * pairs: NULL or host [nframes][2000][2] int32 = (A index, B index) of the matched pairs, -1 padded.
 * The call fails with SG_ERR_GENERIC, writing nothing, when the reference has fewer than 10 stars.
 * Refused before any device work, with a message: SG_ERR_SIZE for nframes < 1, max_stars < 1 or above
 * SG_STARFIT_MAX_STARS; SG_ERR_GENERIC for a missing pointer, ref_image out of range, nstars[f] outside
 * [0, max_stars], a non-finite xpos / ypos / mag among the stars used, an excluded reference.
 * Synchronous.  sg_starmatch_last_times: the last call's device span and launches.
 * sg_starmatch_warp_plan (host only) turns the results into the arguments of sg_warp_frames_u16*, with
 * the loop's failed / skipped bookkeeping: the reference COPY, OK frames APPLY with their hom, every
 * other frame SKIP; out_slot = frame - failed - skipped; *new_total = the frames written.  hom
 * [nframes][9], action, out_slot [nframes]; new_total may be NULL.  Returns 0, or -1 for a missing pointer.
 */
enum { SG_MATCH_OK = 0, SG_MATCH_REFERENCE = 1, SG_MATCH_EXCLUDED = 2, SG_MATCH_FEW_STARS = 3,
       SG_MATCH_NO_TRANS = 4, SG_MATCH_NO_RECALC = 5, SG_MATCH_NO_HOMOGRAPHY = 6 };
#define SG_STARMATCH_MAX_PAIRS 2000	/* MAX_STARS_FITTED */

typedef struct {
	int32_t status, nbpoints, nbright, scale_retry, nwinners, npairs, nr_recalc, inliers, ransac_iters, lm_iters;
	double trans0[6], trans[6], sig, sx, sy, hom[9];
	float fwhmx, fwhmy;
	double shiftx, shifty;
} sg_starmatch_result;

int sg_starmatch(sg_ctx *ctx, int dev_index, int nframes, int max_stars, const int32_t *nstars, const sg_star *stars,
		int ref_image, const uint8_t *included, sg_starmatch_result *results, int32_t *pairs, void *stream);
int sg_starmatch_last_times(sg_ctx *ctx, int dev_index, double *ms, int *launches);
int sg_starmatch_warp_plan(const sg_starmatch_result *results, int nframes, double *hom, int *action, int *out_slot,
		int *new_total);

/* Synthetic sequence generator of include/sg_synth.h on the device (bench / tests):
 * frame f, channel c, row r at d_frames[f*frame_stride + (c*height + r)*width]
 * (frame_stride 0 = nb_layers*height*width). */
int sg_synth_fill_device(sg_ctx *ctx, int dev_index, uint16_t *d_frames, int nframes,
		int nb_layers, int height, int width, int row_begin, int row_end, uint64_t seed,
		int maxshift, int64_t frame_stride, void *stream);
/* the same for frames [first_frame, first_frame + nframes) of the sequence, written from d_frames
 * (a rank's block of a frame-sharded sequence), channel c at c * plane_stride (0 = height *
 * width): row r of channel c of local frame f at d_frames[f*frame_stride + c*plane_stride + r*width]
 * (a band-resident layout passes a base pointer biased by -row_begin*width) */
int sg_synth_fill_frames_device(sg_ctx *ctx, int dev_index, uint16_t *d_frames, int first_frame,
		int nframes, int nb_layers, int height, int width, int row_begin, int row_end, uint64_t seed,
		int maxshift, int64_t frame_stride, int64_t plane_stride, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* SIRILGPU_H */
