"""ctypes binding of libsirilgpu.so (include/sirilgpu.h) for tests, bench.py and smoke().

The product is the C ABI + gfx950 kernels; this module only marshals arguments.  It
refuses to run if the shared library has not been built: there is no Python or CPU
fallback for any pixel.
"""
import ctypes
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
PKG_DIR = os.path.dirname(_HERE)
LIB_PATH = os.environ.get("SG_LIB_PATH") or os.path.join(PKG_DIR, "lib", "libsirilgpu.so")  # A/B builds

# enum values (src/stacking/stacking.c:54-56, src/stacking/stacking.h:14-30)
SUM, MEAN, MEDIAN, MAX, MIN = range(5)
NO_REJEC, PERCENTILE, SIGMA, SIGMEDIAN, WINSORIZED, LINEARFIT = range(6)
NO_NORM, ADDITIVE, MULTIPLICATIVE, ADDITIVE_SCALING, MULTIPLICATIVE_SCALING = range(5)
PATH_AUTO, PATH_SORTED = 0, 1
RESULT_AT_COLLECT = 1        # sg_stack_desc.flags (SG_STACK_RESULT_AT_COLLECT)

SG_OK = 0
SG_ERR_GENERIC, SG_ERR_SIZE, SG_ERR_READ, SG_ERR_DEVICE = -1, -2, -3, -10


class StackDesc(ctypes.Structure):
    _fields_ = [
        ("method", ctypes.c_int),
        ("rejection", ctypes.c_int),
        ("normalize", ctypes.c_int),
        ("sig", ctypes.c_double * 2),
        ("nb_frames", ctypes.c_int),
        ("width", ctypes.c_int),
        ("height", ctypes.c_int),
        ("nb_layers", ctypes.c_int),
        ("shiftx", ctypes.POINTER(ctypes.c_int)),
        ("shifty", ctypes.POINTER(ctypes.c_int)),
        ("offset", ctypes.POINTER(ctypes.c_double)),
        ("mul", ctypes.POINTER(ctypes.c_double)),
        ("scale", ctypes.POINTER(ctypes.c_double)),
        ("max_thread", ctypes.c_int),
        ("max_number_of_rows", ctypes.c_int),
        ("kernel_path", ctypes.c_int),
        ("resident_rows", ctypes.c_int * 2),
        ("flags", ctypes.c_int),
        ("reserved", ctypes.c_int * 2),
    ]


class StackStats(ctypes.Structure):
    _fields_ = [
        ("kernel_ms", ctypes.c_double),
        ("total_ms", ctypes.c_double),
        ("slow_pixels", ctypes.c_uint64),
        ("chain_pixels", ctypes.c_uint64),
        ("launches", ctypes.c_uint64),
        ("main_kernel_blocks", ctypes.c_int),
        ("path", ctypes.c_int),
        ("reg_ties_resolved", ctypes.c_uint64),
        ("reg_ties_unresolved", ctypes.c_uint64),
        ("reg_fp64_reruns", ctypes.c_uint64),
        ("compact_pixels", ctypes.c_uint64),
        ("reg_ms", ctypes.c_double),
        ("norm_fma", ctypes.c_int64),
    ]


class Rect(ctypes.Structure):
    _fields_ = [("x", ctypes.c_int), ("y", ctypes.c_int), ("w", ctypes.c_int), ("h", ctypes.c_int)]


class PreproDesc(ctypes.Structure):
    _fields_ = [("width", ctypes.c_int), ("height", ctypes.c_int), ("nb_layers", ctypes.c_int),
                ("offset", ctypes.c_void_p), ("dark", ctypes.c_void_p), ("flat", ctypes.c_void_p),
                ("dark_optimization", ctypes.c_int), ("cosmetic", ctypes.c_int),
                ("cosme_sigma", ctypes.c_double * 2), ("is_cfa", ctypes.c_int), ("autolevel", ctypes.c_int),
                ("normalisation", ctypes.c_float)]


class PreproInfo(ctypes.Structure):
    _fields_ = [("level", ctypes.c_double), ("icold", ctypes.c_int64), ("ihot", ctypes.c_int64),
                ("thres_cold", ctypes.c_double), ("thres_hot", ctypes.c_double),
                ("dark_sigma", ctypes.c_double), ("dark_median", ctypes.c_double),
                ("cosmetic_applies", ctypes.c_int), ("components", ctypes.c_int64),
                ("longest_component", ctypes.c_int64)]


class FindstarDesc(ctypes.Structure):
    _fields_ = [("width", ctypes.c_int), ("height", ctypes.c_int), ("nb_layers", ctypes.c_int),
                ("layer", ctypes.c_int), ("radius", ctypes.c_int), ("sigma", ctypes.c_double),
                ("use_area", ctypes.c_int), ("area", Rect), ("max_candidates", ctypes.c_int)]


class FindstarFrame(ctypes.Structure):
    _fields_ = [("ngood", ctypes.c_int64), ("median", ctypes.c_double), ("sigma", ctypes.c_double),
                ("threshold", ctypes.c_int), ("ncand", ctypes.c_int64), ("nstored", ctypes.c_int64),
                ("wavelet_applied", ctypes.c_int), ("ratio_applied", ctypes.c_int),
                ("sigma_on_host", ctypes.c_int), ("threshold_wrapped", ctypes.c_int), ("no_data", ctypes.c_int)]


class StarfitDesc(ctypes.Structure):
    _fields_ = [("find", FindstarDesc), ("roundness", ctypes.c_double), ("norm", ctypes.c_double),
                ("fwhm_scale_x", ctypes.c_double), ("fwhm_scale_y", ctypes.c_double),
                ("max_stars", ctypes.c_int), ("want_candidates", ctypes.c_int)]


# sg_star / sg_starfit_cand as numpy structured types; SG_FIT_* are the values of `status`
FIT_FIELDS = ("B", "A", "x0", "y0", "sx", "sy", "fwhmx", "fwhmy", "mag", "rmse", "xpos", "ypos")
STAR_DTYPE = np.dtype([("cand", "<i4"), ("x", "<i4"), ("y", "<i4"), ("iters", "<i4")] + [(k, "<f8") for k in FIT_FIELDS])
CAND_DTYPE = np.dtype([("x", "<i4"), ("y", "<i4"), ("iters", "<i4"), ("status", "<i4"), ("failed_test", "<i4"),
                       ("reserved", "<i4"), ("init", "<f8", (6,))] + [(k, "<f8") for k in FIT_FIELDS])
(SG_FIT_STAR, SG_FIT_NOT_ENOUGH_PIXELS, SG_FIT_NONFINITE, SG_FIT_BAD_FWHM, SG_FIT_NOT_STAR,
 SG_FIT_OVER_CAP) = range(6)
assert STAR_DTYPE.itemsize == 112 and CAND_DTYPE.itemsize == 168


READ_REGION_FN = ctypes.CFUNCTYPE(ctypes.c_int, ctypes.c_void_p, ctypes.c_int, ctypes.c_int,
                                  ctypes.POINTER(ctypes.c_uint16), ctypes.POINTER(Rect))
CONT_FN = ctypes.CFUNCTYPE(ctypes.c_int, ctypes.c_void_p)

class SeqInfo(ctypes.Structure):
    _fields_ = [("width", ctypes.c_int), ("height", ctypes.c_int), ("nb_layers", ctypes.c_int),
                ("nb_frames", ctypes.c_int), ("bytes_per_sample", ctypes.c_int), ("source", ctypes.c_int),
                ("ser_color_id", ctypes.c_int), ("frame_bytes", ctypes.c_int64)]


class EccOut(ctypes.Structure):
    """sg_ecc_out: per-frame host arrays"""
    _fields_ = [("shiftx", ctypes.c_void_p), ("shifty", ctypes.c_void_p), ("dx", ctypes.c_void_p),
                ("dy", ctypes.c_void_p), ("rho", ctypes.c_void_p), ("iterations", ctypes.c_void_p),
                ("failed", ctypes.c_void_p)]


class CosmeDesc(ctypes.Structure):
    _fields_ = [("width", ctypes.c_int), ("height", ctypes.c_int), ("nb_layers", ctypes.c_int),
                ("sig", ctypes.c_double * 2), ("amount", ctypes.c_double), ("is_cfa", ctypes.c_int)]


class CosmeFrame(ctypes.Structure):
    """sg_cosme_frame: one frame's outcome of the automatic cosmetic correction"""
    _fields_ = [("status", ctypes.c_int), ("failed_layer", ctypes.c_int), ("icold", ctypes.c_int64),
                ("ihot", ctypes.c_int64), ("bkg", ctypes.c_double * 3), ("avg_dev", ctypes.c_double * 3)]


class WarpSeqDesc(ctypes.Structure):
    """sg_warp_seq_desc: the shapes of a sequence warp"""
    _fields_ = [("width", ctypes.c_int), ("height", ctypes.c_int), ("nb_layers", ctypes.c_int),
                ("out_width", ctypes.c_int), ("out_height", ctypes.c_int), ("interpolation", ctypes.c_int),
                ("frame_pitch", ctypes.c_int64), ("out_frame_pitch", ctypes.c_int64)]


WARP_SKIP, WARP_APPLY, WARP_COPY = 0, 1, 2


class SeqpsfDesc(ctypes.Structure):
    """sg_seqpsf_desc"""
    _fields_ = [("framing", ctypes.c_int), ("area", Rect), ("norm", ctypes.c_double), ("fwhm_scale_x", ctypes.c_double),
                ("fwhm_scale_y", ctypes.c_double), ("fit_angle", ctypes.c_int)]


SEQPSF_ORIGINAL, SEQPSF_REGISTERED, SEQPSF_FOLLOW_STAR = 0, 1, 2
SEQPSF_NOT_RUN, SEQPSF_EXCLUDED = 6, 7        # statuses beside SG_FIT_* 0 .. 3
SEQPSF_MAX_SIDE = 128
SEQPSF_FIELDS = ("B", "A", "x0", "y0", "sx", "sy", "fwhmx", "fwhmy", "angle", "mag", "rmse", "xpos", "ypos")
# sg_seqpsf_frame as a numpy structured type
SEQPSF_DTYPE = np.dtype([("status", "<i4"), ("angle_fitted", "<i4"), ("iters", "<i4"), ("iters_angle", "<i4"),
                         ("area_x", "<i4"), ("area_y", "<i4"), ("ngood", "<i8"), ("bg", "<f8"), ("init", "<f8", (6,)),
                         ("noangle", "<f8", (6,))] + [(k, "<f8") for k in SEQPSF_FIELDS])
assert SEQPSF_DTYPE.itemsize == 240

# sg_starmatch: statuses, sg_starmatch_result as a numpy structured type, the pairs' capacity per frame
MATCH_OK, MATCH_REFERENCE, MATCH_EXCLUDED, MATCH_FEW_STARS, MATCH_NO_TRANS, MATCH_NO_RECALC, MATCH_NO_HOMOGRAPHY = range(7)
STARMATCH_INT_FIELDS = ("status", "nbpoints", "nbright", "scale_retry", "nwinners", "npairs", "nr_recalc", "inliers",
                        "ransac_iters", "lm_iters")
STARMATCH_DTYPE = np.dtype([(k, "<i4") for k in STARMATCH_INT_FIELDS] +
                           [("trans0", "<f8", (6,)), ("trans", "<f8", (6,)), ("sig", "<f8"), ("sx", "<f8"), ("sy", "<f8"),
                            ("hom", "<f8", (9,)), ("fwhmx", "<f4"), ("fwhmy", "<f4"), ("shiftx", "<f8"), ("shifty", "<f8")])
assert STARMATCH_DTYPE.itemsize == 256
STARMATCH_MAX_PAIRS = 2000


# every symbol include/sirilgpu.h and include/sirilgpu_io.h declare
EXPORTS = ["sg_init", "sg_shutdown", "sg_last_error", "sg_stack_u16", "sg_stack_u16_device",
           "sg_stack_u16_device_async", "sg_stack_collect", "sg_stack_wait_tail", "sg_device_count",
           "sg_get_last_stats", "sg_register_dft_u16", "sg_register_dft_u16_device",
           "sg_register_dft_u16_device_raw", "sg_register_dft_u16_device_pitched", "sg_synth_fill_device",
           "sg_seq_open_ser", "sg_seq_open_fits", "sg_seq_close", "sg_seq_get_info", "sg_seq_read_region",
           "sg_seq_read_frame", "sg_seq_load_device", "sg_seq_set_debayer", "sg_seq_set_debayer_method", "sg_warp_u16", "sg_warp_u16_device",
           "sg_frame_stats_ikss_device", "sg_compute_normalization", "sg_seqfile_read", "sg_seqfile_create",
           "sg_seqfile_free", "sg_seqfile_get_info", "sg_seqfile_get_images", "sg_seqfile_set_image",
           "sg_seqfile_get_registration", "sg_seqfile_set_registration", "sg_seqfile_write",
           "sg_prepro_create", "sg_prepro_free", "sg_prepro_get_info", "sg_prepro_frames_device",
           "sg_prepro_frames", "sg_prepro_noise_device", "sg_findstar_device", "sg_findstar",
           "sg_findstar_fit_device", "sg_findstar_fit", "sg_register_ecc_u16_device", "sg_register_ecc_u16",
           "sg_register_ecc_last_times", "sg_cosme_autodetect_device", "sg_cosme_autodetect", "sg_cosme_last_times",
           "sg_quality_u16_device", "sg_quality_u16", "sg_quality_last_times", "sg_quality_normalize", "sg_quality_select",
           "sg_warp_frames_u16_device", "sg_warp_frames_u16", "sg_warp_frames_last_times",
           "sg_seqpsf_u16_device", "sg_seqpsf_u16", "sg_seqpsf_last_times", "sg_seqpsf_shifts",
           "sg_starmatch", "sg_starmatch_last_times", "sg_starmatch_warp_plan"]
# opencv_interpolation (src/core/siril.h:257-264)
OPENCV_NEAREST, OPENCV_LINEAR, OPENCV_AREA, OPENCV_CUBIC, OPENCV_LANCZOS4 = range(5)

_lib = None


def load():
    """Load libsirilgpu.so; raises if it is missing (fail loudly, no fallback)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(f"{LIB_PATH} not built: run `make -C siril-0.9_amd` (no CPU fallback)")
    lib = ctypes.CDLL(LIB_PATH)
    P = ctypes.c_void_p
    lib.sg_init.argtypes = [ctypes.POINTER(P), ctypes.c_int, ctypes.POINTER(ctypes.c_int)]
    lib.sg_init.restype = ctypes.c_int
    lib.sg_shutdown.argtypes = [P]
    lib.sg_shutdown.restype = None
    lib.sg_last_error.argtypes = [P]
    lib.sg_last_error.restype = ctypes.c_char_p
    lib.sg_stack_u16.argtypes = [P, ctypes.POINTER(StackDesc), READ_REGION_FN, P, CONT_FN, P,
                                 ctypes.POINTER(ctypes.c_uint16), ctypes.POINTER(ctypes.c_uint64),
                                 ctypes.POINTER(ctypes.c_uint64)]
    lib.sg_stack_u16.restype = ctypes.c_int
    lib.sg_stack_u16_device.argtypes = [P, ctypes.c_int, ctypes.POINTER(StackDesc), P, ctypes.c_int64,
                                        ctypes.c_int64, P, ctypes.c_int, ctypes.c_int,
                                        ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_uint64), P]
    lib.sg_stack_u16_device.restype = ctypes.c_int
    lib.sg_stack_u16_device_async.argtypes = [P, ctypes.c_int, ctypes.POINTER(StackDesc), P, ctypes.c_int64,
                                              ctypes.c_int64, P, ctypes.c_int, ctypes.c_int, P]
    lib.sg_stack_u16_device_async.restype = ctypes.c_int
    lib.sg_stack_collect.argtypes = [P, ctypes.c_int, ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_uint64)]
    lib.sg_stack_collect.restype = ctypes.c_int
    lib.sg_stack_wait_tail.argtypes = [P, ctypes.c_int, ctypes.c_void_p]
    lib.sg_stack_wait_tail.restype = ctypes.c_int
    lib.sg_device_count.argtypes = [P, ctypes.POINTER(ctypes.c_int)]
    lib.sg_device_count.restype = ctypes.c_int
    lib.sg_get_last_stats.argtypes = [P, ctypes.POINTER(StackStats)]
    lib.sg_get_last_stats.restype = ctypes.c_int
    lib.sg_synth_fill_device.argtypes = [P, ctypes.c_int, P, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                         ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_uint64,
                                         ctypes.c_int, ctypes.c_int64, P]
    lib.sg_synth_fill_device.restype = ctypes.c_int
    lib.sg_synth_fill_frames_device.argtypes = [P, ctypes.c_int, P, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                                ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                                ctypes.c_uint64, ctypes.c_int, ctypes.c_int64, ctypes.c_int64, P]
    lib.sg_synth_fill_frames_device.restype = ctypes.c_int
    lib.sg_register_dft_u16.argtypes = [P, P, ctypes.c_int, ctypes.c_int, ctypes.c_int, P, P, P, P]
    lib.sg_register_dft_u16.restype = ctypes.c_int
    lib.sg_register_dft_u16_device.argtypes = [P, ctypes.c_int, P, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                               P, P, P, P, P]
    lib.sg_register_dft_u16_device.restype = ctypes.c_int
    lib.sg_register_dft_u16_device_raw.argtypes = lib.sg_register_dft_u16_device.argtypes
    lib.sg_register_dft_u16_device_raw.restype = ctypes.c_int
    lib.sg_register_dft_u16_device_pitched.argtypes = [P, ctypes.c_int, P, ctypes.c_int64, ctypes.c_int64, ctypes.c_int,
                                                       ctypes.c_int, ctypes.c_int, P, P, P, P, ctypes.c_int, P]
    lib.sg_register_dft_u16_device_pitched.restype = ctypes.c_int
    lib.sg_seq_open_ser.argtypes = [ctypes.c_char_p, ctypes.POINTER(P)]
    lib.sg_seq_open_ser.restype = ctypes.c_int
    lib.sg_seq_open_fits.argtypes = [ctypes.POINTER(ctypes.c_char_p), ctypes.c_int, ctypes.POINTER(P)]
    lib.sg_seq_open_fits.restype = ctypes.c_int
    lib.sg_seq_close.argtypes = [P]
    lib.sg_seq_close.restype = None
    lib.sg_seq_get_info.argtypes = [P, ctypes.POINTER(SeqInfo)]
    lib.sg_seq_get_info.restype = ctypes.c_int
    lib.sg_seq_read_region.argtypes = [P, ctypes.c_int, ctypes.c_int, ctypes.POINTER(ctypes.c_uint16),
                                       ctypes.POINTER(Rect)]
    lib.sg_seq_read_region.restype = ctypes.c_int
    lib.sg_seq_read_frame.argtypes = [P, ctypes.c_int, ctypes.POINTER(ctypes.c_uint16)]
    lib.sg_seq_read_frame.restype = ctypes.c_int
    lib.sg_seq_read_selection.argtypes = [P, ctypes.c_int, ctypes.c_int, ctypes.POINTER(Rect),
                                          ctypes.POINTER(ctypes.c_uint16)]
    lib.sg_seq_read_selection.restype = ctypes.c_int
    lib.sg_frame_stats_ikss.argtypes = [P, P, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, P, P]
    lib.sg_frame_stats_ikss.restype = ctypes.c_int
    lib.sg_seq_load_device.argtypes = [P, ctypes.c_int, P, ctypes.c_int, ctypes.c_int, P, ctypes.c_int64, P]
    lib.sg_seq_load_device.restype = ctypes.c_int
    lib.sg_frame_stats_ikss_device.argtypes = [P, ctypes.c_int, P, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                               ctypes.c_int, ctypes.c_int64, P, P, P]
    lib.sg_frame_stats_ikss_device.restype = ctypes.c_int
    lib.sg_compute_normalization.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_int, P, P, P, P, P]
    lib.sg_compute_normalization.restype = ctypes.c_int
    lib.sg_seqfile_read.argtypes = [ctypes.c_char_p, ctypes.POINTER(P)]
    lib.sg_seqfile_create.argtypes = [ctypes.c_char_p, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                      ctypes.c_int, ctypes.c_int, ctypes.POINTER(P)]
    lib.sg_seqfile_free.argtypes = [P]
    lib.sg_seqfile_free.restype = None
    lib.sg_seqfile_get_info.argtypes = [P, ctypes.POINTER(SeqFileInfo)]
    lib.sg_seqfile_get_images.argtypes = [P, P, P, P, P]
    lib.sg_seqfile_set_image.argtypes = [P, ctypes.c_int, ctypes.c_int, ctypes.c_int, P]
    lib.sg_seqfile_get_registration.argtypes = [P, ctypes.c_int, P, P, P, P, P, P, P]
    lib.sg_seqfile_set_registration.argtypes = [P, ctypes.c_int, P, P, P]
    lib.sg_seqfile_write.argtypes = [P, ctypes.c_char_p]
    lib.sg_seq_set_debayer.argtypes = [P, ctypes.c_int]
    lib.sg_seq_set_debayer.restype = ctypes.c_int
    lib.sg_seq_set_debayer_method.argtypes = [P, ctypes.c_int, ctypes.c_int]
    lib.sg_seq_set_debayer_method.restype = ctypes.c_int
    lib.sg_warp_u16.argtypes = [P, P, ctypes.c_int, ctypes.c_int, ctypes.c_int, P, ctypes.c_int, ctypes.c_int,
                                ctypes.POINTER(ctypes.c_double), ctypes.c_int]
    lib.sg_warp_u16.restype = ctypes.c_int
    lib.sg_warp_u16_device.argtypes = [P, ctypes.c_int, P, ctypes.c_int, ctypes.c_int, ctypes.c_int, P, ctypes.c_int,
                                       ctypes.c_int, ctypes.POINTER(ctypes.c_double), ctypes.c_int, P]
    lib.sg_warp_u16_device.restype = ctypes.c_int
    lib.sg_warp_frames_u16_device.argtypes = [P, ctypes.c_int, ctypes.POINTER(WarpSeqDesc), P, ctypes.c_int, P, P, P, P, P]
    lib.sg_warp_frames_u16_device.restype = ctypes.c_int
    lib.sg_warp_frames_u16.argtypes = [P, ctypes.POINTER(WarpSeqDesc), P, ctypes.c_int, P, P, P, P]
    lib.sg_warp_frames_u16.restype = ctypes.c_int
    lib.sg_warp_frames_last_times.argtypes = [P, ctypes.c_int, ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int),
                                              ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_uint64),
                                              ctypes.POINTER(ctypes.c_uint64)]
    lib.sg_warp_frames_last_times.restype = ctypes.c_int
    lib.sg_prepro_create.argtypes = [P, ctypes.c_int, ctypes.POINTER(PreproDesc), ctypes.POINTER(P)]
    lib.sg_prepro_create.restype = ctypes.c_int
    lib.sg_prepro_free.argtypes = [P]
    lib.sg_prepro_free.restype = None
    lib.sg_prepro_get_info.argtypes = [P, ctypes.POINTER(PreproInfo)]
    lib.sg_prepro_get_info.restype = ctypes.c_int
    lib.sg_prepro_frames_device.argtypes = [P, ctypes.c_int, P, P, ctypes.c_int, ctypes.c_int64, P, P]
    lib.sg_prepro_frames_device.restype = ctypes.c_int
    lib.sg_prepro_frames.argtypes = [P, P, P, ctypes.c_int, P]
    lib.sg_prepro_frames.restype = ctypes.c_int
    lib.sg_prepro_noise_device.argtypes = [P, ctypes.c_int, P, P, ctypes.c_int, ctypes.c_int64, P, P, P]
    lib.sg_prepro_noise_device.restype = ctypes.c_int
    lib.sg_findstar_device.argtypes = [P, ctypes.c_int, ctypes.POINTER(FindstarDesc), P, ctypes.c_int, ctypes.c_int64,
                                       ctypes.POINTER(FindstarFrame), P, P, P, P]
    lib.sg_findstar_device.restype = ctypes.c_int
    lib.sg_findstar.argtypes = [P, ctypes.POINTER(FindstarDesc), P, ctypes.c_int, ctypes.POINTER(FindstarFrame), P, P, P]
    lib.sg_findstar.restype = ctypes.c_int
    lib.sg_findstar_fit_device.argtypes = [P, ctypes.c_int, ctypes.POINTER(StarfitDesc), P, ctypes.c_int, ctypes.c_int64,
                                           ctypes.POINTER(FindstarFrame), P, P, P, P]
    lib.sg_findstar_fit_device.restype = ctypes.c_int
    lib.sg_findstar_fit.argtypes = [P, ctypes.POINTER(StarfitDesc), P, ctypes.c_int, ctypes.POINTER(FindstarFrame), P, P, P]
    lib.sg_findstar_fit.restype = ctypes.c_int
    lib.sg_register_ecc_u16_device.argtypes = [P, ctypes.c_int, P, ctypes.c_int64, ctypes.c_int64, ctypes.c_int,
                                               ctypes.c_int, ctypes.c_int, ctypes.c_int, P, ctypes.POINTER(EccOut), P]
    lib.sg_register_ecc_u16_device.restype = ctypes.c_int
    lib.sg_register_ecc_u16.argtypes = [P, P, ctypes.c_int64, ctypes.c_int64, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                        ctypes.c_int, P, ctypes.POINTER(EccOut)]
    lib.sg_register_ecc_u16.restype = ctypes.c_int
    lib.sg_register_ecc_last_times.argtypes = [P, ctypes.c_int, ctypes.POINTER(ctypes.c_double),
                                               ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int)]
    lib.sg_register_ecc_last_times.restype = ctypes.c_int
    lib.sg_cosme_autodetect_device.argtypes = [P, ctypes.c_int, ctypes.POINTER(CosmeDesc), P, ctypes.c_int, ctypes.c_int64,
                                               P, ctypes.POINTER(CosmeFrame)]
    lib.sg_cosme_autodetect_device.restype = ctypes.c_int
    lib.sg_cosme_autodetect.argtypes = [P, ctypes.POINTER(CosmeDesc), P, ctypes.c_int, ctypes.POINTER(CosmeFrame)]
    lib.sg_cosme_autodetect.restype = ctypes.c_int
    lib.sg_cosme_last_times.argtypes = [P, ctypes.c_int, ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_double),
                                        ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int),
                                        ctypes.POINTER(ctypes.c_int64)]
    lib.sg_cosme_last_times.restype = ctypes.c_int
    lib.sg_quality_u16_device.argtypes = [P, ctypes.c_int, P, ctypes.c_int64, ctypes.c_int64, ctypes.c_int, ctypes.c_int,
                                          ctypes.c_int, P, P, P]
    lib.sg_quality_u16_device.restype = ctypes.c_int
    lib.sg_quality_u16.argtypes = [P, P, ctypes.c_int64, ctypes.c_int64, ctypes.c_int, ctypes.c_int, ctypes.c_int, P, P]
    lib.sg_quality_u16.restype = ctypes.c_int
    lib.sg_quality_last_times.argtypes = [P, ctypes.c_int, ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int),
                                          ctypes.POINTER(ctypes.c_int)]
    lib.sg_quality_last_times.restype = ctypes.c_int
    lib.sg_quality_normalize.argtypes = [ctypes.c_int, ctypes.c_int, P, P, P, P, ctypes.POINTER(ctypes.c_double),
                                         ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int), ctypes.c_char_p,
                                         ctypes.c_int]
    lib.sg_quality_normalize.restype = ctypes.c_int
    lib.sg_quality_select.argtypes = [ctypes.c_int, P, P, ctypes.c_double, ctypes.POINTER(ctypes.c_double), P,
                                      ctypes.POINTER(ctypes.c_int), ctypes.c_char_p, ctypes.c_int]
    lib.sg_quality_select.restype = ctypes.c_int
    lib.sg_seqpsf_u16_device.argtypes = [P, ctypes.c_int, ctypes.POINTER(SeqpsfDesc), P, ctypes.c_int64, ctypes.c_int64,
                                         ctypes.c_int, ctypes.c_int, ctypes.c_int, P, P, P, P, ctypes.POINTER(Rect), P]
    lib.sg_seqpsf_u16_device.restype = ctypes.c_int
    lib.sg_seqpsf_u16.argtypes = [P, ctypes.POINTER(SeqpsfDesc), P, ctypes.c_int64, ctypes.c_int64, ctypes.c_int,
                                  ctypes.c_int, ctypes.c_int, P, P, P, P, ctypes.POINTER(Rect)]
    lib.sg_seqpsf_u16.restype = ctypes.c_int
    lib.sg_seqpsf_last_times.argtypes = [P, ctypes.c_int, ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int)]
    lib.sg_seqpsf_last_times.restype = ctypes.c_int
    lib.sg_seqpsf_shifts.argtypes = [ctypes.c_int, ctypes.c_int, P, P, P, P, ctypes.POINTER(ctypes.c_int),
                                     ctypes.POINTER(ctypes.c_double)]
    lib.sg_seqpsf_shifts.restype = ctypes.c_int
    lib.sg_starmatch.argtypes = [P, ctypes.c_int, ctypes.c_int, ctypes.c_int, P, P, ctypes.c_int, P, P, P, P]
    lib.sg_starmatch.restype = ctypes.c_int
    lib.sg_starmatch_last_times.argtypes = [P, ctypes.c_int, ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int)]
    lib.sg_starmatch_last_times.restype = ctypes.c_int
    lib.sg_starmatch_warp_plan.argtypes = [P, ctypes.c_int, P, P, P, ctypes.POINTER(ctypes.c_int)]
    lib.sg_starmatch_warp_plan.restype = ctypes.c_int
    _lib = lib
    return lib


class SeqFileInfo(ctypes.Structure):
    _fields_ = [("name", ctypes.c_char * 512), ("beg", ctypes.c_int), ("number", ctypes.c_int),
                ("selnum", ctypes.c_int), ("fixed", ctypes.c_int), ("reference_image", ctypes.c_int),
                ("type", ctypes.c_int), ("nb_layers", ctypes.c_int)]


SEQFILE_REGULAR, SEQFILE_SER, SEQFILE_FILM = 0, 1, 2


class SeqFile:
    """A Siril .seq file (include/sirilgpu_io.h sg_seqfile_*): host-only."""

    def __init__(self, handle):
        self.lib = load()
        self.h = handle

    @classmethod
    def read(cls, path):
        lib = load()
        h = ctypes.c_void_p()
        rc = lib.sg_seqfile_read(os.fsencode(path), ctypes.byref(h))
        if rc != SG_OK:
            raise OSError(f"sg_seqfile_read({path}) failed ({rc})")
        return cls(h)

    @classmethod
    def create(cls, name, number, beg=1, fixed=5, reference_image=-1, type=SEQFILE_REGULAR, nb_layers=1):
        lib = load()
        h = ctypes.c_void_p()
        rc = lib.sg_seqfile_create(name.encode(), beg, number, fixed, reference_image, type, nb_layers, ctypes.byref(h))
        if rc != SG_OK:
            raise RuntimeError(f"sg_seqfile_create failed ({rc})")
        return cls(h)

    def close(self):
        if self.h:
            self.lib.sg_seqfile_free(self.h)
            self.h = None

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def info(self):
        i = SeqFileInfo()
        self.lib.sg_seqfile_get_info(self.h, ctypes.byref(i))
        return i

    def images(self):
        n = self.info().number
        fn, inc, hs = (np.zeros(n, np.int32) for _ in range(3))
        st = np.zeros((n, 10), np.float64)
        self.lib.sg_seqfile_get_images(self.h, fn.ctypes.data_as(ctypes.c_void_p), inc.ctypes.data_as(ctypes.c_void_p),
                                       hs.ctypes.data_as(ctypes.c_void_p), st.ctypes.data_as(ctypes.c_void_p))
        return fn, inc, hs, st

    def set_image(self, index, filenum, incl, stats=None):
        st = None if stats is None else np.ascontiguousarray(stats, dtype=np.float64)
        rc = self.lib.sg_seqfile_set_image(self.h, index, filenum, incl,
                                           None if st is None else st.ctypes.data_as(ctypes.c_void_p))
        if rc != SG_OK:
            raise RuntimeError("sg_seqfile_set_image failed")

    def registration(self, layer):
        """(rc, shiftx, shifty, rot_centre_x, rot_centre_y, angle, fwhm, quality); rc 1 = no data"""
        n = self.info().number
        sx, sy = np.zeros(n, np.int32), np.zeros(n, np.int32)
        fl = [np.zeros(n, np.float32) for _ in range(4)]
        q = np.zeros(n, np.float64)
        rc = self.lib.sg_seqfile_get_registration(self.h, layer, sx.ctypes.data_as(ctypes.c_void_p),
                                                  sy.ctypes.data_as(ctypes.c_void_p),
                                                  *[a.ctypes.data_as(ctypes.c_void_p) for a in fl],
                                                  q.ctypes.data_as(ctypes.c_void_p))
        return (rc, sx, sy, *fl, q)

    def set_registration(self, layer, shiftx, shifty, quality=None):
        sx = np.ascontiguousarray(shiftx, dtype=np.int32)
        sy = np.ascontiguousarray(shifty, dtype=np.int32)
        q = None if quality is None else np.ascontiguousarray(quality, dtype=np.float64)
        rc = self.lib.sg_seqfile_set_registration(self.h, layer, sx.ctypes.data_as(ctypes.c_void_p),
                                                  sy.ctypes.data_as(ctypes.c_void_p),
                                                  None if q is None else q.ctypes.data_as(ctypes.c_void_p))
        if rc != SG_OK:
            raise RuntimeError("sg_seqfile_set_registration failed")

    def write(self, path):
        rc = self.lib.sg_seqfile_write(self.h, os.fsencode(path))
        if rc != SG_OK:
            raise OSError(f"sg_seqfile_write({path}) failed ({rc})")


# sensor_pattern (src/core/siril.h:266-271)
BAYER_RGGB, BAYER_BGGR, BAYER_GBRG, BAYER_GRBG = 0, 1, 2, 3
# interpolation_method (src/core/siril.h:249-255)
BAYER_INTER_BILINEAR, BAYER_INTER_NEARESTNEIGHBOR, BAYER_INTER_VNG, BAYER_INTER_AHD, BAYER_INTER_SUPER_PIXEL = range(5)


class Seq:
    """An opened SER file or FITS sequence (include/sirilgpu_io.h); host-side reads need no GPU."""

    def __init__(self, handle):
        self.lib = load()
        self.h = handle
        info = SeqInfo()
        rc = self.lib.sg_seq_get_info(self.h, ctypes.byref(info))
        if rc != SG_OK:
            raise RuntimeError(f"sg_seq_get_info failed ({rc})")
        self.info = info
        self.shape = (info.nb_frames, info.nb_layers, info.height, info.width)

    @classmethod
    def open_ser(cls, path):
        lib = load()
        h = ctypes.c_void_p()
        rc = lib.sg_seq_open_ser(os.fsencode(path), ctypes.byref(h))
        if rc != SG_OK:
            raise OSError(f"sg_seq_open_ser({path}) failed ({rc})")
        return cls(h)

    @classmethod
    def open_fits(cls, paths):
        lib = load()
        arr = (ctypes.c_char_p * len(paths))(*[os.fsencode(p) for p in paths])
        h = ctypes.c_void_p()
        rc = lib.sg_seq_open_fits(arr, len(paths), ctypes.byref(h))
        if rc != SG_OK:
            raise OSError(f"sg_seq_open_fits failed ({rc})")
        return cls(h)

    def close(self):
        if self.h:
            self.lib.sg_seq_close(self.h)
            self.h = None

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def set_debayer(self, pattern=-1, interpolation=BAYER_INTER_BILINEAR):
        """demosaic a CFA SER on host reads and device loads; pattern BAYER_* or -1 = from the
        header; interpolation BAYER_INTER_BILINEAR, _NEARESTNEIGHBOR or _VNG (AHD and super-pixel
        are refused, see include/sirilgpu_io.h)"""
        rc = self.lib.sg_seq_set_debayer_method(self.h, pattern, interpolation)
        if rc != SG_OK:
            raise RuntimeError(f"sg_seq_set_debayer_method failed ({rc})")
        info = SeqInfo()
        self.lib.sg_seq_get_info(self.h, ctypes.byref(info))
        self.info = info
        self.shape = (info.nb_frames, info.nb_layers, info.height, info.width)

    def read_region(self, layer, index, x, y, w, h):
        """top-down band (seq_opened_read_region); returns (rc, array[h][w])"""
        buf = np.zeros((h, w), dtype=np.uint16)
        rc = self.lib.sg_seq_read_region(self.h, layer, index, buf.ctypes.data_as(ctypes.POINTER(ctypes.c_uint16)),
                                         ctypes.byref(Rect(x, y, w, h)))
        return rc, buf

    def read_selection(self, layer, index, x, y, w, h):
        """seq_read_frame_part: the selection (display coordinates) bottom-up; (rc, array[h][w])"""
        buf = np.zeros((h, w), dtype=np.uint16)
        rc = self.lib.sg_seq_read_selection(self.h, layer, index, ctypes.byref(Rect(x, y, w, h)),
                                            buf.ctypes.data_as(ctypes.POINTER(ctypes.c_uint16)))
        return rc, buf

    def read_frame(self, index):
        out = np.zeros(self.shape[1:], dtype=np.uint16)
        rc = self.lib.sg_seq_read_frame(self.h, index, out.ctypes.data_as(ctypes.POINTER(ctypes.c_uint16)))
        if rc != SG_OK:
            raise RuntimeError(f"sg_seq_read_frame({index}) failed ({rc})")
        return out


def _iptr(a):
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_int)) if a is not None else None


def _dptr(a):
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_double)) if a is not None else None


def make_desc(method, N, W, H, C, rejection=NO_REJEC, normalize=NO_NORM, sig=(4.0, 3.0),
              shiftx=None, shifty=None, offset=None, mul=None, scale=None, max_thread=8,
              max_number_of_rows=0, kernel_path=PATH_AUTO, resident_rows=None, flags=0):
    """Build a StackDesc; returns (desc, keepalive) -- keep the arrays alive during the call.
    resident_rows = (first, end) memory rows present at the device frames (None = all)."""
    keep = []

    def arr(a, dt):
        if a is None:
            return None
        a = np.ascontiguousarray(a, dtype=dt)
        keep.append(a)
        return a

    sx, sy = arr(shiftx, np.int32), arr(shifty, np.int32)
    of, mu, sc = arr(offset, np.float64), arr(mul, np.float64), arr(scale, np.float64)
    d = StackDesc()
    d.method, d.rejection, d.normalize = method, rejection, normalize
    d.sig[0], d.sig[1] = float(sig[0]), float(sig[1])
    d.nb_frames, d.width, d.height, d.nb_layers = N, W, H, C
    d.shiftx, d.shifty = _iptr(sx), _iptr(sy)
    d.offset, d.mul, d.scale = _dptr(of), _dptr(mu), _dptr(sc)
    d.max_thread, d.max_number_of_rows = max_thread, max_number_of_rows
    d.kernel_path = kernel_path
    d.flags = flags
    if resident_rows is not None:
        d.resident_rows[0], d.resident_rows[1] = int(resident_rows[0]), int(resident_rows[1])
    return d, keep


def make_findstar_desc(W, H, C, layer, radius, sigma, area=None, max_candidates=2000):
    d = FindstarDesc()
    d.width, d.height, d.nb_layers, d.layer = W, H, C, layer
    d.radius, d.sigma, d.max_candidates = radius, sigma, max_candidates
    d.use_area = 0 if area is None else 1
    if area is not None:
        d.area.x, d.area.y, d.area.w, d.area.h = [int(v) for v in area]
    return d


def make_starfit_desc(W, H, C, layer, radius, sigma, area=None, max_candidates=2000, roundness=0.5, norm=65535.0,
                      fwhm_scales=(1.0, 1.0), max_stars=2000, want_candidates=False):
    d = StarfitDesc()
    d.find = make_findstar_desc(W, H, C, layer, radius, sigma, area, max_candidates)
    d.roundness, d.norm = roundness, norm
    d.fwhm_scale_x, d.fwhm_scale_y = fwhm_scales
    d.max_stars, d.want_candidates = max_stars, int(bool(want_candidates))
    return d


def make_cosme_desc(W, H, C, sig=(3.0, 3.0), amount=1.0, is_cfa=False):
    """sg_cosme_desc: sig = (cold, hot), -1 switches a test off"""
    d = CosmeDesc()
    d.width, d.height, d.nb_layers = W, H, C
    d.sig[0], d.sig[1] = float(sig[0]), float(sig[1])
    d.amount, d.is_cfa = float(amount), int(bool(is_cfa))
    return d


def _starfit_arrays(nframes, max_candidates, max_stars, want_candidates):
    n = max(nframes, 0)
    nstars = np.zeros(n, dtype=np.int32)
    stars = np.zeros((n, max(max_stars, 0)), dtype=STAR_DTYPE)
    cands = np.zeros((n, max(max_candidates, 0)), dtype=CAND_DTYPE) if want_candidates else None
    return nstars, stars, cands


def _findstar_arrays(nframes, radius, max_candidates, want_boxes):
    n, m, r2 = max(nframes, 0), max(max_candidates, 0), 2 * max(radius, 0)
    xy = np.zeros((n, m, 2), dtype=np.int32)
    bx = np.zeros((n, m, r2, r2), dtype=np.uint16) if want_boxes else None
    return xy, bx


class Context:
    def __init__(self, devices=None):
        self.lib = load()
        self.ctx = ctypes.c_void_p()
        if devices:
            arr = (ctypes.c_int * len(devices))(*devices)
            rc = self.lib.sg_init(ctypes.byref(self.ctx), len(devices), arr)
        else:
            rc = self.lib.sg_init(ctypes.byref(self.ctx), 0, None)
        if rc != SG_OK:
            raise RuntimeError(f"sg_init failed ({rc})")

    def close(self):
        if self.ctx:
            self.lib.sg_shutdown(self.ctx)
            self.ctx = ctypes.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def error(self):
        return self.lib.sg_last_error(self.ctx).decode()

    def check(self, rc, what):
        if rc != SG_OK:
            raise RuntimeError(f"{what} failed ({rc}): {self.error()}")

    def stats(self):
        st = StackStats()
        self.check(self.lib.sg_get_last_stats(self.ctx, ctypes.byref(st)), "sg_get_last_stats")
        return st

    def stack_device(self, desc, d_frames, frame_stride, plane_stride, d_out, row_begin, row_end,
                     stream=None, dev_index=0):
        rej = (ctypes.c_uint64 * 6)()
        maxim = ctypes.c_uint64(0)
        rc = self.lib.sg_stack_u16_device(self.ctx, dev_index, ctypes.byref(desc), ctypes.c_void_p(d_frames),
                                          frame_stride, plane_stride, ctypes.c_void_p(d_out), row_begin,
                                          row_end, rej, ctypes.byref(maxim),
                                          ctypes.c_void_p(stream) if stream else None)
        self.check(rc, "sg_stack_u16_device")
        return np.array(list(rej), dtype=np.uint64).reshape(3, 2), int(maxim.value)

    def stack_device_async(self, desc, d_frames, frame_stride, plane_stride, d_out, row_begin, row_end,
                           stream=None, dev_index=0):
        """sg_stack_u16_device_async: queued, nothing waited for; results via collect()"""
        rc = self.lib.sg_stack_u16_device_async(self.ctx, dev_index, ctypes.byref(desc), ctypes.c_void_p(d_frames),
                                                frame_stride, plane_stride, ctypes.c_void_p(d_out), row_begin,
                                                row_end, ctypes.c_void_p(stream) if stream else None)
        self.check(rc, "sg_stack_u16_device_async")

    def wait_tail(self, stream=None, dev_index=0):
        """sg_stack_wait_tail: work queued on `stream` from now on waits for the async calls' tail kernels"""
        self.check(self.lib.sg_stack_wait_tail(self.ctx, dev_index, ctypes.c_void_p(stream) if stream else None),
                   "sg_stack_wait_tail")

    def collect(self, dev_index=0):
        """sg_stack_collect: (rc, summed rejection counters [3][2], max SUM maximum) of the pending calls"""
        rej = (ctypes.c_uint64 * 6)()
        maxim = ctypes.c_uint64(0)
        rc = self.lib.sg_stack_collect(self.ctx, dev_index, rej, ctypes.byref(maxim))
        return rc, np.array(list(rej), dtype=np.uint64).reshape(3, 2), int(maxim.value)

    def device_count(self):
        n = ctypes.c_int(0)
        self.check(self.lib.sg_device_count(self.ctx, ctypes.byref(n)), "sg_device_count")
        return n.value

    def load_seq_device(self, seq, d_frames, first=0, count=None, frame_stride=0, dev_index=0, stream=None):
        """frames of an opened Seq decoded on the device (sg_seq_load_device)"""
        if count is None:
            count = seq.shape[0] - first
        rc = self.lib.sg_seq_load_device(self.ctx, dev_index, seq.h, first, count, ctypes.c_void_p(d_frames),
                                         frame_stride, ctypes.c_void_p(stream) if stream else None)
        self.check(rc, "sg_seq_load_device")

    def frame_stats_ikss(self, d_frames, nframes, C, H, W, frame_stride=0, dev_index=0, stream=None):
        """per-frame IKSS location / scale of layer 0 (sg_frame_stats_ikss_device);
        returns (rc, location[nframes], scale[nframes])"""
        loc = np.zeros(nframes, dtype=np.float64)
        scl = np.zeros(nframes, dtype=np.float64)
        rc = self.lib.sg_frame_stats_ikss_device(self.ctx, dev_index, ctypes.c_void_p(d_frames), nframes, C, H, W,
                                                 frame_stride, loc.ctypes.data_as(ctypes.c_void_p),
                                                 scl.ctypes.data_as(ctypes.c_void_p),
                                                 ctypes.c_void_p(stream) if stream else None)
        return rc, loc, scl

    def frame_stats_ikss_host(self, frames):
        """the same statistics of host frames [N][C][H][W] u16 (sg_frame_stats_ikss);
        returns (rc, location[N], scale[N])"""
        frames = np.ascontiguousarray(frames, dtype=np.uint16)
        N, C, H, W = frames.shape
        loc = np.zeros(N, dtype=np.float64)
        scl = np.zeros(N, dtype=np.float64)
        rc = self.lib.sg_frame_stats_ikss(self.ctx, frames.ctypes.data_as(ctypes.c_void_p), N, C, H, W,
                                          loc.ctypes.data_as(ctypes.c_void_p), scl.ctypes.data_as(ctypes.c_void_p))
        return rc, loc, scl

    def warp(self, image, hom, out_size=None, interpolation=OPENCV_LINEAR):
        """cvTransformImage on a memory-order image [C][H][W]; hom = the 3x3 homography
        (Homography h00..h22), out_size = (ref.x, ref.y)"""
        image = np.ascontiguousarray(image, dtype=np.uint16)
        C, H, W = image.shape
        oW, oH = out_size if out_size else (W, H)
        out = np.zeros((C, oH, oW), dtype=np.uint16)
        h = (ctypes.c_double * 9)(*[float(v) for v in np.asarray(hom, dtype=np.float64).reshape(9)])
        rc = self.lib.sg_warp_u16(self.ctx, image.ctypes.data_as(ctypes.c_void_p), W, H, C,
                                  out.ctypes.data_as(ctypes.c_void_p), oW, oH, h, interpolation)
        self.check(rc, "sg_warp_u16")
        return out

    def warp_device(self, d_in, W, H, C, d_out, oW, oH, hom, interpolation, stream=None, dev_index=0):
        """the same on a resident image: d_in [C][H][W] -> d_out [C][oH][oW], device pointers
        (sg_warp_u16_device).  With a stream the call returns once the kernel is queued on it."""
        h = (ctypes.c_double * 9)(*[float(v) for v in np.asarray(hom, dtype=np.float64).reshape(9)])
        rc = self.lib.sg_warp_u16_device(self.ctx, dev_index, ctypes.c_void_p(d_in), W, H, C, ctypes.c_void_p(d_out),
                                         oW, oH, h, interpolation, ctypes.c_void_p(stream) if stream else None)
        self.check(rc, "sg_warp_u16_device")

    @staticmethod
    def _warp_seq_args(nframes, hom, action, out_slot):
        h = np.ascontiguousarray(hom, dtype=np.float64).reshape(-1)
        if h.size != 9 * max(nframes, 0):
            raise ValueError("hom: one 3x3 homography per frame")
        a = None if action is None else np.ascontiguousarray(action, dtype=np.int32)
        s = None if out_slot is None else np.ascontiguousarray(out_slot, dtype=np.int32)
        if (a is not None and a.size != nframes) or (s is not None and s.size != nframes):
            raise ValueError("action / out_slot: one entry per frame")
        return h, a, s

    def warp_frames_device(self, d_in, nframes, W, H, C, d_out, oW, oH, hom, interpolation, action=None, out_slot=None,
                           frame_pitch=0, out_frame_pitch=0, stream=None, dev_index=0):
        """cvTransformImage on every frame of a resident sequence, one homography each (sg_warp_frames_u16_device):
        frame f = C planes of W x H at d_in + f * frame_pitch elements (0 = tight), hom [nframes][3][3]; action[f]
        WARP_SKIP / WARP_APPLY / WARP_COPY (None = all APPLY); the result goes to output frame out_slot[f] (None = f)
        at d_out + out_slot[f] * out_frame_pitch elements.  Returns rc; with a stream, once the work is queued on it."""
        h, a, s = self._warp_seq_args(nframes, hom, action, out_slot)
        d = WarpSeqDesc(W, H, C, oW, oH, interpolation, frame_pitch, out_frame_pitch)
        P = ctypes.c_void_p
        return self.lib.sg_warp_frames_u16_device(self.ctx, dev_index, ctypes.byref(d), P(d_in), nframes, h.ctypes.data_as(P),
                                                  a.ctypes.data_as(P) if a is not None else None,
                                                  s.ctypes.data_as(P) if s is not None else None, P(d_out),
                                                  P(stream) if stream else None)

    def warp_frames(self, frames, hom, out_size=None, interpolation=OPENCV_LINEAR, action=None, out_slot=None, out=None):
        """the same on host frames [N][C][H][W] (sg_warp_frames_u16).  Returns (rc, out): out [slots][C][oH][oW], a new
        zero array with a slot per frame unless one is passed in (u16, C-contiguous); only written frames are touched."""
        frames = np.ascontiguousarray(frames, dtype=np.uint16)
        N, C, H, W = frames.shape
        oW, oH = out_size if out_size else (W, H)
        h, a, s = self._warp_seq_args(N, hom, action, out_slot)
        if out is None:
            out = np.zeros((N, C, oH, oW), dtype=np.uint16)
        if out.dtype != np.uint16 or not out.flags.c_contiguous or out.shape[1:] != (C, oH, oW):
            raise ValueError("out: a C-contiguous u16 array [slots][C][oH][oW]")
        written = [f if s is None else int(s[f]) for f in range(N) if a is None or a[f] != WARP_SKIP]
        if written and max(written) >= out.shape[0]:
            raise ValueError("out: fewer frames than the largest slot")
        d = WarpSeqDesc(W, H, C, oW, oH, interpolation, 0, 0)
        P = ctypes.c_void_p
        rc = self.lib.sg_warp_frames_u16(self.ctx, ctypes.byref(d), frames.ctypes.data_as(P), N, h.ctypes.data_as(P),
                                         a.ctypes.data_as(P) if a is not None else None,
                                         s.ctypes.data_as(P) if s is not None else None, out.ctypes.data_as(P))
        return rc, out

    def warp_frames_last_times(self, dev_index=0):
        """(device ms, kernel launches, tiles_lds, tiles_gather, pixels_stray) of the last sequence warp on that device,
        after waiting for it"""
        ms, n = ctypes.c_double(), ctypes.c_int()
        a, b, c = ctypes.c_uint64(), ctypes.c_uint64(), ctypes.c_uint64()
        self.check(self.lib.sg_warp_frames_last_times(self.ctx, dev_index, ctypes.byref(ms), ctypes.byref(n), ctypes.byref(a),
                                                      ctypes.byref(b), ctypes.byref(c)), "sg_warp_frames_last_times")
        return ms.value, n.value, a.value, b.value, c.value

    def stack_seq(self, desc, seq):
        """Host-pull stack whose pull callback is the library's own sg_seq_read_region (C),
        i.e. stack_mean_with_rejection & co. reading the sequence's files directly."""
        N, C, H, W = seq.shape
        rf = ctypes.cast(self.lib.sg_seq_read_region, READ_REGION_FN)
        cf = CONT_FN(lambda user: 1)
        out = np.zeros((C, H, W), dtype=np.uint16)
        rej = (ctypes.c_uint64 * 6)()
        maxim = ctypes.c_uint64(0)
        rc = self.lib.sg_stack_u16(self.ctx, ctypes.byref(desc), rf, seq.h, cf, None,
                                   out.ctypes.data_as(ctypes.POINTER(ctypes.c_uint16)), rej,
                                   ctypes.byref(maxim))
        return rc, out, np.array(list(rej), dtype=np.uint64).reshape(3, 2), int(maxim.value)

    def stack_host(self, desc, frames, cancel_after=None):
        """Host-pull path: frames[N][C][H][W] (memory order) served through a
        seq_opened_read_region-shaped callback returning top-down bands."""
        N, C, H, W = frames.shape
        calls = [0]

        def read_region(user, layer, index, buf, area):
            a = area.contents
            band = frames[index, layer, H - 1 - (a.y + np.arange(a.h)), a.x:a.x + a.w]
            dst = np.ctypeslib.as_array(buf, shape=(a.h * a.w,))
            dst[:] = np.ascontiguousarray(band).reshape(-1)
            return 0

        def cont(user):
            calls[0] += 1
            return 0 if (cancel_after is not None and calls[0] > cancel_after) else 1

        rf, cf = READ_REGION_FN(read_region), CONT_FN(cont)
        out = np.zeros((C, H, W), dtype=np.uint16)
        rej = (ctypes.c_uint64 * 6)()
        maxim = ctypes.c_uint64(0)
        rc = self.lib.sg_stack_u16(self.ctx, ctypes.byref(desc), rf, None, cf, None,
                                   out.ctypes.data_as(ctypes.POINTER(ctypes.c_uint16)), rej,
                                   ctypes.byref(maxim))
        return rc, out, np.array(list(rej), dtype=np.uint64).reshape(3, 2), int(maxim.value)

    def register_dft(self, sel, ref_image=0, included=None):
        """register_shift_dft on host selections sel[nframes][S][S] (bottom-up, one layer)."""
        sel = np.ascontiguousarray(sel, dtype=np.uint16)
        n, S, S2 = sel.shape
        assert S == S2
        inc = None if included is None else np.ascontiguousarray(included, dtype=np.int32)
        sx = np.zeros(n, dtype=np.int32)
        sy = np.zeros(n, dtype=np.int32)
        q = np.zeros(n, dtype=np.float64)
        P = ctypes.c_void_p
        rc = self.lib.sg_register_dft_u16(self.ctx, sel.ctypes.data_as(P), n, S, ref_image,
                                          inc.ctypes.data_as(P) if inc is not None else None,
                                          sx.ctypes.data_as(P), sy.ctypes.data_as(P), q.ctypes.data_as(P))
        self.check(rc, "sg_register_dft_u16")
        return sx, sy, q

    def register_dft_device(self, d_sel, nframes, S, ref_image=0, included=None, stream=None, dev_index=0,
                            raw_quality=False, frame_pitch=0, row_pitch=0):
        """register_shift_dft on device selections; raw_quality: the shard entry point
        (sg_register_dft_u16_device_raw: QualityEstimate values, not normalised); frame_pitch /
        row_pitch (elements): selections read in place from resident frames
        (sg_register_dft_u16_device_pitched)"""
        inc = None if included is None else np.ascontiguousarray(included, dtype=np.int32)
        sx = np.zeros(nframes, dtype=np.int32)
        sy = np.zeros(nframes, dtype=np.int32)
        q = np.zeros(nframes, dtype=np.float64)
        P = ctypes.c_void_p
        args = (inc.ctypes.data_as(P) if inc is not None else None, sx.ctypes.data_as(P), sy.ctypes.data_as(P),
                q.ctypes.data_as(P))
        if frame_pitch or row_pitch:
            rc = self.lib.sg_register_dft_u16_device_pitched(
                self.ctx, dev_index, P(d_sel), frame_pitch or S * S, row_pitch or S, nframes, S, ref_image, *args,
                1 if raw_quality else 0, P(stream) if stream else None)
            self.check(rc, "sg_register_dft_u16_device_pitched")
            return sx, sy, q
        fn = self.lib.sg_register_dft_u16_device_raw if raw_quality else self.lib.sg_register_dft_u16_device
        rc = fn(self.ctx, dev_index, P(d_sel), nframes, S, ref_image, *args, P(stream) if stream else None)
        self.check(rc, "sg_register_dft_u16_device" + ("_raw" if raw_quality else ""))
        return sx, sy, q

    @staticmethod
    def _ecc_arrays(nframes):
        res = {"shiftx": np.zeros(nframes, dtype=np.int32), "shifty": np.zeros(nframes, dtype=np.int32),
               "dx": np.zeros(nframes, dtype=np.float32), "dy": np.zeros(nframes, dtype=np.float32),
               "rho": np.zeros(nframes, dtype=np.float64), "iterations": np.zeros(nframes, dtype=np.int32),
               "failed": np.zeros(nframes, dtype=np.int32)}
        out = EccOut(*[res[k].ctypes.data for k, _ in EccOut._fields_])
        return res, out

    def register_ecc_device(self, d_frames, nframes, H, W, ref_image=0, included=None, frame_pitch=0, row_pitch=0,
                            stream=None, dev_index=0):
        """register_ecc's per-frame work on resident frames read in place (sg_register_ecc_u16_device): frame f,
        row r at d_frames + f * frame_pitch + r * row_pitch elements (0 = tight).  Returns (rc, dict of the
        per-frame arrays shiftx, shifty, dx, dy, rho, iterations, failed); frames outside `included` keep 0."""
        inc = None if included is None else np.ascontiguousarray(included, dtype=np.int32)
        res, out = self._ecc_arrays(nframes)
        P = ctypes.c_void_p
        rc = self.lib.sg_register_ecc_u16_device(self.ctx, dev_index, P(d_frames), frame_pitch, row_pitch, W, H, nframes,
                                                 ref_image, inc.ctypes.data_as(P) if inc is not None else None,
                                                 ctypes.byref(out), P(stream) if stream else None)
        return rc, res

    def register_ecc_last_times(self, dev_index=0):
        """(prepare ms, iterate ms, iteration launches) of the last ECC call on that device"""
        a, b, n = ctypes.c_double(), ctypes.c_double(), ctypes.c_int()
        self.check(self.lib.sg_register_ecc_last_times(self.ctx, dev_index, ctypes.byref(a), ctypes.byref(b),
                                                       ctypes.byref(n)), "sg_register_ecc_last_times")
        return a.value, b.value, n.value

    def register_ecc(self, frames, ref_image=0, included=None, layer=0):
        """the same on host frames [N][H][W] or [N][C][H][W] u16, layer `layer` (sg_register_ecc_u16)"""
        frames = np.ascontiguousarray(frames, dtype=np.uint16)
        if frames.ndim == 3:
            frames = frames[:, None]
        N, C, H, W = frames.shape
        inc = None if included is None else np.ascontiguousarray(included, dtype=np.int32)
        res, out = self._ecc_arrays(N)
        P = ctypes.c_void_p
        base = frames.ctypes.data + layer * H * W * 2
        rc = self.lib.sg_register_ecc_u16(self.ctx, P(base), C * H * W, W, W, H, N, ref_image,
                                          inc.ctypes.data_as(P) if inc is not None else None, ctypes.byref(out))
        return rc, res

    @staticmethod
    def _seqpsf_args(nframes, area, framing, included, reg_shifts, norm, scales, fit_angle, carry):
        d = SeqpsfDesc(framing, Rect(*[int(v) for v in area]), norm, scales[0], scales[1], 1 if fit_angle else 0)
        inc = None if included is None else np.ascontiguousarray(included, dtype=np.int32)
        rsx = rsy = None
        if reg_shifts is not None:
            rsx = np.ascontiguousarray(reg_shifts[0], dtype=np.int32)
            rsy = np.ascontiguousarray(reg_shifts[1], dtype=np.int32)
        rec = np.zeros(max(nframes, 1), dtype=SEQPSF_DTYPE)
        cx, cy = carry if carry is not None else area[:2]      # the chain starts at the area unless told otherwise
        cr = Rect(int(cx), int(cy), int(area[2]), int(area[3]))
        P = ctypes.c_void_p
        ptr = lambda a: a.ctypes.data_as(P) if a is not None else None
        return d, rec, cr, (ptr(inc), ptr(rsx), ptr(rsy)), (inc, rsx, rsy)

    def seqpsf_device(self, d_frames, nframes, H, W, area, framing=SEQPSF_ORIGINAL, included=None, reg_shifts=None,
                      norm=65535.0, scales=(1.0, 1.0), fit_angle=True, carry=None, frame_pitch=0, row_pitch=0, stream=None,
                      dev_index=0):
        """seqpsf's per-frame work on resident frames read in place (sg_seqpsf_u16_device): the PSF of the star
        in `area` = (x, y, w, h), display coordinates, of every included frame.  reg_shifts = (shiftx, shifty) for
        SEQPSF_REGISTERED; carry = (x, y) starts a SEQPSF_FOLLOW_STAR chain there instead of at the area.
        Returns (rc, records as a SEQPSF_DTYPE array, the carried area (x, y))."""
        d, rec, cr, ptrs, keep = self._seqpsf_args(nframes, area, framing, included, reg_shifts, norm, scales, fit_angle, carry)
        P = ctypes.c_void_p
        rc = self.lib.sg_seqpsf_u16_device(self.ctx, dev_index, ctypes.byref(d), P(d_frames), frame_pitch, row_pitch, W, H,
                                           nframes, ptrs[0], ptrs[1], ptrs[2], rec.ctypes.data_as(P),
                                           ctypes.byref(cr), P(stream) if stream else None)
        return rc, rec[:max(nframes, 0)], (cr.x, cr.y)

    def seqpsf(self, frames, area, framing=SEQPSF_ORIGINAL, included=None, reg_shifts=None, norm=65535.0,
               scales=(1.0, 1.0), fit_angle=True, carry=None, layer=0):
        """the same on host frames [N][H][W] or [N][C][H][W] u16, layer `layer` (sg_seqpsf_u16)"""
        frames = np.ascontiguousarray(frames, dtype=np.uint16)
        if frames.ndim == 3:
            frames = frames[:, None]
        N, C, H, W = frames.shape
        d, rec, cr, ptrs, keep = self._seqpsf_args(N, area, framing, included, reg_shifts, norm, scales, fit_angle, carry)
        P = ctypes.c_void_p
        rc = self.lib.sg_seqpsf_u16(self.ctx, ctypes.byref(d), P(frames.ctypes.data + layer * H * W * 2), C * H * W, W, W, H, N,
                                    ptrs[0], ptrs[1], ptrs[2], rec.ctypes.data_as(P), ctypes.byref(cr))
        return rc, rec[:N], (cr.x, cr.y)

    def seqpsf_last_times(self, dev_index=0):
        """(device ms, kernel launches) of the last seqpsf call on that device; after seqpsf(), summed over its batches"""
        a, n = ctypes.c_double(), ctypes.c_int()
        self.check(self.lib.sg_seqpsf_last_times(self.ctx, dev_index, ctypes.byref(a), ctypes.byref(n)), "sg_seqpsf_last_times")
        return a.value, n.value

    def starmatch(self, nstars, stars, ref_image=0, included=None, want_pairs=False, stream=None, dev_index=0):
        """new_star_match of every frame's star list against the reference frame's (sg_starmatch): nstars [N] and
        stars [N][max_stars] of STAR_DTYPE as findstar_fit returns them.  Returns (results as a STARMATCH_DTYPE
        array, pairs [N][2000][2] int32 of (A index, B index), -1 padded, or None).  Raises on a refusal and when
        the reference frame has fewer than 10 stars; the message is the library's."""
        nstars = np.ascontiguousarray(nstars, dtype=np.int32)
        stars = np.ascontiguousarray(stars, dtype=STAR_DTYPE)
        n = len(nstars)
        max_stars = stars.shape[1] if stars.ndim == 2 else 0
        if stars.ndim != 2 or stars.shape[0] != n:
            raise ValueError("stars must be [len(nstars)][max_stars]")
        inc = None if included is None else np.ascontiguousarray(included, dtype=np.uint8)
        if inc is not None and len(inc) != n:
            raise ValueError("included must have one entry per frame")
        res = np.zeros(max(n, 1), dtype=STARMATCH_DTYPE)
        pairs = np.full((max(n, 1), STARMATCH_MAX_PAIRS, 2), -1, dtype=np.int32) if want_pairs else None
        P = ctypes.c_void_p
        rc = self.lib.sg_starmatch(self.ctx, dev_index, n, max_stars, nstars.ctypes.data_as(P), stars.ctypes.data_as(P), ref_image,
                                   inc.ctypes.data_as(P) if inc is not None else None, res.ctypes.data_as(P),
                                   pairs.ctypes.data_as(P) if pairs is not None else None, P(stream) if stream else None)
        self.check(rc, "sg_starmatch")
        return res[:n], (pairs[:n] if pairs is not None else None)

    def starmatch_last_times(self, dev_index=0):
        """(device ms, kernel launches) of the last starmatch call on that device"""
        a, n = ctypes.c_double(), ctypes.c_int()
        self.check(self.lib.sg_starmatch_last_times(self.ctx, dev_index, ctypes.byref(a), ctypes.byref(n)), "sg_starmatch_last_times")
        return a.value, n.value

    def cosme_autodetect_device(self, d_frames, nframes, C, H, W, sig=(3.0, 3.0), amount=1.0, is_cfa=False,
                                frame_stride=0, stream=None, dev_index=0):
        """seqfind_cosme's per-frame work (autoDetect on every layer) on resident frames, in place
        (sg_cosme_autodetect_device); returns (rc, list of CosmeFrame)"""
        d = make_cosme_desc(W, H, C, sig, amount, is_cfa)
        rec = (CosmeFrame * max(nframes, 1))()
        rc = self.lib.sg_cosme_autodetect_device(self.ctx, dev_index, ctypes.byref(d), ctypes.c_void_p(d_frames), nframes,
                                                 frame_stride, ctypes.c_void_p(stream) if stream else None, rec)
        return rc, list(rec)[:max(nframes, 0)]

    def cosme_autodetect(self, frames, sig=(3.0, 3.0), amount=1.0, is_cfa=False):
        """the same on host frames [N][C][H][W] u16, corrected in place (sg_cosme_autodetect); returns
        (rc, list of CosmeFrame)"""
        assert frames.dtype == np.uint16 and frames.flags.c_contiguous and frames.flags.writeable and frames.ndim == 4
        N, C, H, W = frames.shape
        d = make_cosme_desc(W, H, C, sig, amount, is_cfa)
        rec = (CosmeFrame * max(N, 1))()
        rc = self.lib.sg_cosme_autodetect(self.ctx, ctypes.byref(d), frames.ctypes.data_as(ctypes.c_void_p), N, rec)
        return rc, list(rec)[:N]

    def cosme_last_times(self, dev_index=0):
        """(statistics ms, main pass ms, dependence resolution ms, rounds, pixels re-examined) of the last
        cosmetic correction call on that device"""
        a, b, c = ctypes.c_double(), ctypes.c_double(), ctypes.c_double()
        n, m = ctypes.c_int(), ctypes.c_int64()
        self.check(self.lib.sg_cosme_last_times(self.ctx, dev_index, ctypes.byref(a), ctypes.byref(b), ctypes.byref(c),
                                                ctypes.byref(n), ctypes.byref(m)), "sg_cosme_last_times")
        return a.value, b.value, c.value, n.value, m.value

    def quality_device(self, d_frames, nframes, H, W, included=None, frame_pitch=0, row_pitch=0, stream=None, dev_index=0,
                       fill=0.0):
        """QualityEstimate of W x H planes resident in HBM, read in place (sg_quality_u16_device): frame f, row r at
        d_frames + f * frame_pitch + r * row_pitch elements (0 = tight).  Returns (rc, quality_raw[nframes]);
        frames outside `included` keep `fill`."""
        inc = None if included is None else np.ascontiguousarray(included, dtype=np.int32)
        q = np.full(max(nframes, 0), fill, dtype=np.float64)
        P = ctypes.c_void_p
        rc = self.lib.sg_quality_u16_device(self.ctx, dev_index, P(d_frames), frame_pitch, row_pitch, W, H, nframes,
                                            inc.ctypes.data_as(P) if inc is not None else None,
                                            q.ctypes.data_as(P) if q.size else None, P(stream) if stream else None)
        return rc, q

    def quality(self, frames, included=None, layer=0, fill=0.0):
        """the same on host frames [N][H][W] or [N][C][H][W] u16, layer `layer` (sg_quality_u16)"""
        frames = np.ascontiguousarray(frames, dtype=np.uint16)
        if frames.ndim == 3:
            frames = frames[:, None]
        N, C, H, W = frames.shape
        inc = None if included is None else np.ascontiguousarray(included, dtype=np.int32)
        q = np.full(N, fill, dtype=np.float64)
        P = ctypes.c_void_p
        rc = self.lib.sg_quality_u16(self.ctx, P(frames.ctypes.data + layer * H * W * 2), C * H * W, W, W, H, N,
                                     inc.ctypes.data_as(P) if inc is not None else None, q.ctypes.data_as(P))
        return rc, q

    def quality_last_times(self, dev_index=0):
        """(device ms, route: 0 none / 1 resident / 2 tiled, kernel launches) of the last quality call on that device"""
        a, r, n = ctypes.c_double(), ctypes.c_int(), ctypes.c_int()
        self.check(self.lib.sg_quality_last_times(self.ctx, dev_index, ctypes.byref(a), ctypes.byref(r), ctypes.byref(n)),
                   "sg_quality_last_times")
        return a.value, r.value, n.value

    def prepro_frames_device(self, prepro, d_frames, nframes, frame_stride=0, want_k=True, stream=None, dev_index=0):
        """seqpreprocess's loop body on resident frames, in place (sg_prepro_frames_device); returns
        (rc, dark_k[nframes] or None)"""
        k = np.zeros(nframes, dtype=np.float64) if want_k else None
        rc = self.lib.sg_prepro_frames_device(self.ctx, dev_index, prepro.h, ctypes.c_void_p(d_frames), nframes,
                                              frame_stride, k.ctypes.data_as(ctypes.c_void_p) if want_k else None,
                                              ctypes.c_void_p(stream) if stream else None)
        return rc, k

    def prepro_frames_host(self, prepro, frames, want_k=True):
        """the same on host frames [N][C][H][W], calibrated in place (sg_prepro_frames); returns (rc, dark_k)"""
        assert frames.dtype == np.uint16 and frames.flags.c_contiguous and frames.flags.writeable
        k = np.zeros(frames.shape[0], dtype=np.float64) if want_k else None
        rc = self.lib.sg_prepro_frames(self.ctx, prepro.h, frames.ctypes.data_as(ctypes.c_void_p), frames.shape[0],
                                       k.ctypes.data_as(ctypes.c_void_p) if want_k else None)
        return rc, k

    def prepro_noise_device(self, prepro, d_frames, nframes, k, frame_stride=0, stream=None, dev_index=0):
        """the dark fit's objective of frame f at k[f] (sg_prepro_noise_device); returns (rc, noise[nframes])"""
        k = np.ascontiguousarray(k, dtype=np.float64)
        assert k.shape == (nframes,)
        noise = np.zeros(nframes, dtype=np.float64)
        rc = self.lib.sg_prepro_noise_device(self.ctx, dev_index, prepro.h, ctypes.c_void_p(d_frames), nframes,
                                             frame_stride, k.ctypes.data_as(ctypes.c_void_p),
                                             noise.ctypes.data_as(ctypes.c_void_p),
                                             ctypes.c_void_p(stream) if stream else None)
        return rc, noise

    def findstar_device(self, d_frames, nframes, C, H, W, radius, sigma, layer=0, area=None, max_candidates=2000,
                        want_boxes=True, d_wave=None, frame_stride=0, stream=None, dev_index=0):
        """peaker's whole-image part on resident frames (sg_findstar_device).  area = (x, y, w, h) in display
        coordinates or None; d_wave = a device pointer for the detection planes [nframes][H][W] or None.
        Returns (rc, records, cand_xy[nframes][max][2] int32, boxes[nframes][max][2r][2r] uint16 or None);
        records is a list of FindstarFrame, boxes[f][i][ii][jj] is the gsl_matrix element (ii, jj)."""
        d = make_findstar_desc(W, H, C, layer, radius, sigma, area, max_candidates)
        rec = (FindstarFrame * max(nframes, 1))()
        xy, bx = _findstar_arrays(nframes, radius, max_candidates, want_boxes)
        rc = self.lib.sg_findstar_device(self.ctx, dev_index, ctypes.byref(d), ctypes.c_void_p(d_frames), nframes,
                                         frame_stride, rec, xy.ctypes.data_as(ctypes.c_void_p),
                                         bx.ctypes.data_as(ctypes.c_void_p) if want_boxes else None,
                                         ctypes.c_void_p(d_wave) if d_wave else None,
                                         ctypes.c_void_p(stream) if stream else None)
        return rc, list(rec)[:max(nframes, 0)], xy, bx

    def findstar(self, frames, radius, sigma, layer=0, area=None, max_candidates=2000, want_boxes=True,
                 want_wave=False):
        """the same on host frames [N][C][H][W] u16 (sg_findstar); returns (rc, records, cand_xy, boxes or None,
        wave[N][H][W] or None)"""
        frames = np.ascontiguousarray(frames, dtype=np.uint16)
        N, C, H, W = frames.shape
        d = make_findstar_desc(W, H, C, layer, radius, sigma, area, max_candidates)
        rec = (FindstarFrame * max(N, 1))()
        xy, bx = _findstar_arrays(N, radius, max_candidates, want_boxes)
        wave = np.zeros((N, H, W), dtype=np.uint16) if want_wave else None
        rc = self.lib.sg_findstar(self.ctx, ctypes.byref(d), frames.ctypes.data_as(ctypes.c_void_p), N, rec,
                                  xy.ctypes.data_as(ctypes.c_void_p),
                                  bx.ctypes.data_as(ctypes.c_void_p) if want_boxes else None,
                                  wave.ctypes.data_as(ctypes.c_void_p) if want_wave else None)
        return rc, list(rec)[:N], xy, bx, wave

    def findstar_fit_device(self, d_frames, nframes, C, H, W, radius, sigma, layer=0, area=None, max_candidates=2000,
                            roundness=0.5, norm=65535.0, fwhm_scales=(1.0, 1.0), max_stars=2000,
                            want_candidates=False, frame_stride=0, stream=None, dev_index=0):
        """all of peaker on resident frames (sg_findstar_fit_device): candidates, PSF fit, is_star, sorted
        star list.  Returns (rc, records, nstars[nframes] int32, stars[nframes][max_stars] of STAR_DTYPE,
        cands[nframes][max_candidates] of CAND_DTYPE or None); frame f's stars are stars[f, :nstars[f]],
        sorted by (mag, cand), its candidate records cands[f, :records[f].nstored]."""
        d = make_starfit_desc(W, H, C, layer, radius, sigma, area, max_candidates, roundness, norm, fwhm_scales,
                              max_stars, want_candidates)
        rec = (FindstarFrame * max(nframes, 1))()
        nstars, stars, cands = _starfit_arrays(nframes, max_candidates, max_stars, want_candidates)
        rc = self.lib.sg_findstar_fit_device(self.ctx, dev_index, ctypes.byref(d), ctypes.c_void_p(d_frames), nframes,
                                             frame_stride, rec, nstars.ctypes.data_as(ctypes.c_void_p),
                                             stars.ctypes.data_as(ctypes.c_void_p),
                                             cands.ctypes.data_as(ctypes.c_void_p) if want_candidates else None,
                                             ctypes.c_void_p(stream) if stream else None)
        return rc, list(rec)[:max(nframes, 0)], nstars, stars, cands

    def findstar_fit(self, frames, radius, sigma, layer=0, area=None, max_candidates=2000, roundness=0.5,
                     norm=65535.0, fwhm_scales=(1.0, 1.0), max_stars=2000, want_candidates=False):
        """the same on host frames [N][C][H][W] u16 (sg_findstar_fit)"""
        frames = np.ascontiguousarray(frames, dtype=np.uint16)
        N, C, H, W = frames.shape
        d = make_starfit_desc(W, H, C, layer, radius, sigma, area, max_candidates, roundness, norm, fwhm_scales,
                              max_stars, want_candidates)
        rec = (FindstarFrame * max(N, 1))()
        nstars, stars, cands = _starfit_arrays(N, max_candidates, max_stars, want_candidates)
        rc = self.lib.sg_findstar_fit(self.ctx, ctypes.byref(d), frames.ctypes.data_as(ctypes.c_void_p), N, rec,
                                      nstars.ctypes.data_as(ctypes.c_void_p), stars.ctypes.data_as(ctypes.c_void_p),
                                      cands.ctypes.data_as(ctypes.c_void_p) if want_candidates else None)
        return rc, list(rec)[:N], nstars, stars, cands

    def synth_fill(self, d_frames, nframes, C, H, W, row_begin, row_end, seed, maxshift, dev_index=0,
                   frame_stride=0, first_frame=0, plane_stride=0):
        rc = self.lib.sg_synth_fill_frames_device(self.ctx, dev_index, ctypes.c_void_p(d_frames), first_frame, nframes,
                                                  C, H, W, row_begin, row_end, seed, maxshift, frame_stride,
                                                  plane_stride, None)
        self.check(rc, "sg_synth_fill_frames_device")


class Prepro:
    """The per-sequence part of seqpreprocess (sg_prepro_create): masters [C][H][W] u16 or None."""

    def __init__(self, ctx, width, height, nb_layers, offset=None, dark=None, flat=None, dark_optimization=False,
                 cosmetic=False, cosme_sigma=(-1.0, -1.0), is_cfa=False, autolevel=False, normalisation=1.0,
                 dev_index=0):
        self.lib = ctx.lib
        self.h = ctypes.c_void_p()
        keep = []

        def master(a):
            if a is None:
                return None
            a = np.ascontiguousarray(a, dtype=np.uint16)
            assert a.size == nb_layers * height * width, "a master has the frames' shape"
            keep.append(a)
            return a.ctypes.data

        d = PreproDesc()
        d.width, d.height, d.nb_layers = width, height, nb_layers
        d.offset, d.dark, d.flat = master(offset), master(dark), master(flat)
        d.dark_optimization, d.cosmetic = int(dark_optimization), int(cosmetic)
        d.cosme_sigma[0], d.cosme_sigma[1] = float(cosme_sigma[0]), float(cosme_sigma[1])
        d.is_cfa, d.autolevel, d.normalisation = int(is_cfa), int(autolevel), float(normalisation)
        self.rc = self.lib.sg_prepro_create(ctx.ctx, dev_index, ctypes.byref(d), ctypes.byref(self.h))
        if self.rc != SG_OK:
            self.h = None
            raise RuntimeError(f"sg_prepro_create failed ({self.rc}): {ctx.error()}")

    def info(self):
        i = PreproInfo()
        rc = self.lib.sg_prepro_get_info(self.h, ctypes.byref(i))
        if rc != SG_OK:
            raise RuntimeError(f"sg_prepro_get_info failed ({rc})")
        return i

    def close(self):
        if self.h:
            self.lib.sg_prepro_free(self.h)
            self.h = None

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()


def seqpsf_shifts(records, ref_image=0):
    """register_shift_fwhm's second step from seqpsf's records (sg_seqpsf_shifts, host only).  Returns (rc, shiftx,
    shifty, fwhm, best index, best fwhm); rc = 1: a frame has no PSF (the reference aborts), -1: the reference frame
    is excluded; the arrays are then None"""
    rec = np.ascontiguousarray(records, dtype=SEQPSF_DTYPE)
    n = len(rec)
    sx, sy, fw = np.zeros(n, dtype=np.int32), np.zeros(n, dtype=np.int32), np.zeros(n, dtype=np.float64)
    bi, bf = ctypes.c_int(-1), ctypes.c_double(0.0)
    P = ctypes.c_void_p
    rc = load().sg_seqpsf_shifts(n, ref_image, rec.ctypes.data_as(P), sx.ctypes.data_as(P), sy.ctypes.data_as(P),
                                 fw.ctypes.data_as(P), ctypes.byref(bi), ctypes.byref(bf))
    if rc != 0:
        return rc, None, None, None, None, None
    return rc, sx, sy, fw, bi.value, bf.value


def starmatch_warp_plan(results):
    """the arguments of warp_frames from starmatch's results (sg_starmatch_warp_plan, host only), with the loop's
    failed / skipped bookkeeping: (hom [N][9], action [N], out_slot [N], new_total)"""
    rec = np.ascontiguousarray(results, dtype=STARMATCH_DTYPE)
    n = len(rec)
    hom, action, slot = np.zeros((n, 9), dtype=np.float64), np.zeros(n, dtype=np.int32), np.zeros(n, dtype=np.int32)
    total = ctypes.c_int(0)
    P = ctypes.c_void_p
    rc = load().sg_starmatch_warp_plan(rec.ctypes.data_as(P), n, hom.ctypes.data_as(P), action.ctypes.data_as(P),
                                       slot.ctypes.data_as(P), ctypes.byref(total))
    if rc != 0:
        raise RuntimeError("sg_starmatch_warp_plan refused its arguments")
    return hom, action, slot, total.value


def compute_normalization(mode, location, scale, ref_image=0):
    """compute_normalization (stacking.c:125-190) through the C ABI: (offset, mul, scale)"""
    lib = load()
    n = len(location)
    loc = np.ascontiguousarray(location, dtype=np.float64)
    sc = np.ascontiguousarray(scale, dtype=np.float64)
    off, mul, so = (np.zeros(n), np.zeros(n), np.zeros(n))
    rc = lib.sg_compute_normalization(mode, n, ref_image, loc.ctypes.data_as(ctypes.c_void_p),
                                      sc.ctypes.data_as(ctypes.c_void_p), off.ctypes.data_as(ctypes.c_void_p),
                                      mul.ctypes.data_as(ctypes.c_void_p), so.ctypes.data_as(ctypes.c_void_p))
    if rc != SG_OK:
        raise RuntimeError(f"sg_compute_normalization failed ({rc})")
    return off, mul, so


def _mask(a, n):
    return None if a is None else np.ascontiguousarray(np.asarray(a).astype(bool), dtype=np.int32).reshape(n)


def normalize_quality(quality_raw, ref_image=0, measured=None, normalized=None):
    """register_ecc's q_min / q_max / q_index bookkeeping and normalizeQualityData through the C ABI
    (sg_quality_normalize): returns (quality, q_min, q_max, q_index)"""
    lib = load()
    raw = np.ascontiguousarray(quality_raw, dtype=np.float64)
    n = raw.size
    mea, nor = _mask(measured, n), _mask(normalized, n)
    q = np.zeros(n, dtype=np.float64)
    lo, hi, idx = ctypes.c_double(), ctypes.c_double(), ctypes.c_int()
    msg = ctypes.create_string_buffer(256)
    P = ctypes.c_void_p
    rc = lib.sg_quality_normalize(n, ref_image, raw.ctypes.data_as(P), mea.ctypes.data_as(P) if mea is not None else None,
                                  nor.ctypes.data_as(P) if nor is not None else None, q.ctypes.data_as(P),
                                  ctypes.byref(lo), ctypes.byref(hi), ctypes.byref(idx), msg, len(msg))
    if rc != SG_OK:
        raise ValueError(f"sg_quality_normalize failed ({rc}): {msg.value.decode()}")
    return q, lo.value, hi.value, idx.value


def select_by_quality(quality, percent, included=None):
    """the "best percent % of the frames" filter through the C ABI (sg_quality_select): returns
    (threshold, indices of the selected frames); raises ValueError where the reference reads outside its
    array or sorts a NaN"""
    lib = load()
    q = np.ascontiguousarray(quality, dtype=np.float64)
    n = q.size
    inc = _mask(included, n)
    sel = np.zeros(max(n, 1), dtype=np.int32)
    thr, cnt = ctypes.c_double(), ctypes.c_int()
    msg = ctypes.create_string_buffer(256)
    P = ctypes.c_void_p
    rc = lib.sg_quality_select(n, q.ctypes.data_as(P), inc.ctypes.data_as(P) if inc is not None else None, float(percent),
                               ctypes.byref(thr), sel.ctypes.data_as(P), ctypes.byref(cnt), msg, len(msg))
    if rc != SG_OK:
        raise ValueError(f"sg_quality_select failed ({rc}): {msg.value.decode()}")
    return thr.value, sel[:cnt.value].copy()
