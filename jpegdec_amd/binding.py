"""ctypes binding of include/jpegdec_amd.h (the C-ABI).  Plumbing only."""
import ctypes as C
import os

import numpy as np

# constants = include/jpegdec_amd.h (= the reference's src/JPEGDEC.h values)
RGB565_LE, RGB565_BE, RGB8888, GRAY8 = 0, 1, 2, 3
FOUR_BIT_DITHERED, TWO_BIT_DITHERED, ONE_BIT_DITHERED = 4, 5, 6      # made from a GRAY8 canvas: dither_surfaces / decode_dither_to_host
DITHER_SEED_BYTES = 2184
SCALE_HALF, SCALE_QUARTER, SCALE_EIGHTH, LUMA_ONLY = 2, 4, 8, 64
PROGRESSIVE_FULL = 256      # ours: every scan of a progressive file at full size (decode_to_host); no effect on a baseline file
PACK_HWC, PACK_CHW, PACK_BGR = 0, 1, 2      # pack_surfaces / decode_packed_to_host: layout flags (PACK_BGR is OR-ed in)
PACK_U8, PACK_F16, PACK_F32 = 0, 1, 2       # .. element types
PACK_DTYPES = {PACK_U8: np.uint8, PACK_F16: np.float16, PACK_F32: np.float32}
ENCODE_GRAY, ENCODE_444, ENCODE_422, ENCODE_420 = 0, 1, 2, 3           # jda_encode_job.sampling
ENCODE_OPTIMIZE = 1                                                    # a job's word of jda_encode_surfaces_ex: Huffman tables of the file's own
ENCODE_SAMPLINGS = {"gray": ENCODE_GRAY, "4:4:4": ENCODE_444, "4:2:2": ENCODE_422, "4:2:0": ENCODE_420}
RESIZE_BILINEAR, RESIZE_BOX, RESIZE_HAMMING, RESIZE_BICUBIC, RESIZE_LANCZOS = range(5)      # JDA_RESIZE_*: Pillow's five convolution filters
RESIZE_FILTERS = {"bilinear": RESIZE_BILINEAR, "box": RESIZE_BOX, "hamming": RESIZE_HAMMING, "bicubic": RESIZE_BICUBIC, "lanczos": RESIZE_LANCZOS}
RESIZE_MAX_KSIZE, RESIZE_MAX_TABLE_BYTES = 161, 64 << 20      # resize_surfaces: taps per output coordinate (a downscale of 80 : 1), tap tables of one call
AUTO_ROTATE = 1      # the class's decode() applies the EXIF orientation; the C-ABI takes it as an argument (decode_oriented_to_host, orient_surfaces)

ERROR_NAMES = {0: "JDA_SUCCESS", 1: "JDA_INVALID_PARAMETER", 2: "JDA_DECODE_ERROR",
               3: "JDA_UNSUPPORTED_FEATURE", 4: "JDA_INVALID_FILE", 5: "JDA_ERROR_MEMORY",
               6: "JDA_ERROR_NO_DEVICE", 7: "JDA_ERROR_HIP"}


class JdaError(RuntimeError):
    def __init__(self, code, what=""):
        self.code = code
        super().__init__("%s (%d) %s" % (ERROR_NAMES.get(code, "?"), code, what))


class ImageInfo(C.Structure):
    _fields_ = [(n, C.c_int32) for n in (
        "width", "height", "ncomp", "subsample", "bpp", "jpeg_type", "restart_interval",
        "orientation", "mcu_w", "mcu_h", "mcus_x", "mcus_y", "scan_offset", "blocks_per_mcu",
        "has_thumb", "thumb_w", "thumb_h", "thumb_offset", "scan_start", "scan_end", "approx")]

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


class ThumbnailSteps(C.Structure):
    """jda_thumbnail_steps"""
    _fields_ = [("out_w", C.c_int32), ("out_h", C.c_int32), ("scale", C.c_int32), ("draft_w", C.c_int32), ("draft_h", C.c_int32), ("fx", C.c_int32), ("fy", C.c_int32),
                ("reduce_box", C.c_int32 * 4), ("reduced_w", C.c_int32), ("reduced_h", C.c_int32), ("resize", C.c_int32), ("box", C.c_float * 4)]


class Output(C.Structure):
    _fields_ = [("pixels", C.c_void_p), ("pitch_bytes", C.c_int32), ("width_px", C.c_int32),
                ("rows", C.c_int32)]


class EncodeJob(C.Structure):
    _fields_ = [(k, C.c_int32) for k in ("x", "y", "w", "h", "sampling", "quality", "restart_interval", "reserved")]


class RecodeSource(C.Structure):
    _fields_ = [("image", C.c_void_p), ("coef", C.c_void_p)]


class RecodeJob(C.Structure):
    _fields_ = [(k, C.c_int32) for k in ("form", "restart_interval", "reserved0", "reserved1")]


class RecodeXform(C.Structure):
    _fields_ = [("op", C.c_int32), ("flags", C.c_int32), ("mcu_rect", C.c_int32 * 4)]


RECODE_BASELINE, RECODE_OPTIMIZE, RECODE_PROGRESSIVE = 0, 1, 2
XF_NONE, XF_FLIP_H, XF_FLIP_V, XF_TRANSPOSE, XF_TRANSVERSE, XF_ROT_90, XF_ROT_180, XF_ROT_270, XF_EXIF = range(9)
XF_TRIM = 1
RECODE_TRANSFORMS = {None: XF_NONE, "none": XF_NONE, "flip_h": XF_FLIP_H, "flip_v": XF_FLIP_V, "transpose": XF_TRANSPOSE, "transverse": XF_TRANSVERSE, "rot90": XF_ROT_90,
                     "rot180": XF_ROT_180, "rot270": XF_ROT_270, "exif": XF_EXIF}
RECODE_FORMS = {"baseline": RECODE_BASELINE, "optimize": RECODE_OPTIMIZE, "progressive": RECODE_PROGRESSIVE}


class PipelineStats(C.Structure):
    _fields_ = [(n, C.c_int64) for n in ("images", "device_images", "host_path_images", "failed_images", "source_pixels",
                                          "compressed_bytes", "h2d_bytes")] + [("launches", C.c_int32), ("spec_rounds_max", C.c_int32)]


class BatchStats(C.Structure):
    _fields_ = [("source_pixels", C.c_int64), ("output_bytes", C.c_int64), ("scan_bytes", C.c_int64),
                ("index_bytes", C.c_int64), ("table_bytes", C.c_int64), ("n_launches", C.c_int32),
                ("n_workgroups", C.c_int32), ("tiles", C.c_int64), ("tiles_whole_images", C.c_int64)]


def library_path() -> str:
    # JDA_LIBRARY: another build of the same library (kernel A/B runs on the GPU box, tools/gpu_ab.sh)
    return os.environ.get("JDA_LIBRARY") or os.path.join(os.path.dirname(os.path.abspath(__file__)), "libjpegdec_amd.so")


_lib = None

# every symbol include/jpegdec_amd.h declares: (name, restype, argtypes)
_P = C.c_void_p
_PROTOTYPES = [
    ("jda_parse", C.c_int, [C.c_char_p, C.c_int32, C.POINTER(ImageInfo)]),
    ("jda_prepare", _P, [C.c_char_p, C.c_int32, C.POINTER(C.c_int32)]),
    ("jda_prepare_ex", _P, [C.c_char_p, C.c_int32, C.c_int32, C.POINTER(C.c_int32)]),
    ("jda_set_host_prescan_helpers", C.c_int, [C.c_int32]),
    ("jda_image_prescan_pending", C.c_int, [_P]),
    ("jda_prepare_batch", C.c_int, [C.c_int32, C.POINTER(C.c_char_p), C.POINTER(C.c_int32), C.c_int32, C.c_int32, C.POINTER(_P), C.POINTER(C.c_int32)]),
    ("jda_dev_image_prescan_on_device", C.c_int, [_P]),
    ("jda_last_prescan_rounds", C.c_int, [_P]),
    ("jda_filter_on_device", C.c_int, [_P, _P, C.c_int32, _P, _P, _P, C.c_int32, _P]),
    ("jda_effective_options", C.c_int32, [_P, C.c_int32]),
    ("jda_dev_image_read_index", C.c_int, [_P, _P, _P, _P]),
    ("jda_dev_image_mcus_ok", C.c_uint32, [_P]),
    ("jda_upload_batch", C.c_int, [_P, C.c_int32, C.POINTER(_P), C.POINTER(_P)]),
    ("jda_image_free", None, [_P]),
    ("jda_image_get_info", C.POINTER(ImageInfo), [_P]),
    ("jda_image_scan", _P, [_P, C.POINTER(C.c_uint32)]),
    ("jda_image_block_index", _P, [_P, C.POINTER(C.c_uint32)]),
    ("jda_image_block_dc", _P, [_P]),
    ("jda_index_equivalent", C.c_int, [_P, _P, C.c_uint32]),
    ("jda_image_block_cont", _P, [_P, C.POINTER(_P), C.POINTER(C.c_uint32)]),
    ("jda_kernel_launch_counts", C.c_int, [C.c_char_p, C.c_int]),
    ("jda_image_tables", _P, [_P, C.POINTER(C.c_uint32)]),
    ("jda_image_truncation_events", C.c_uint32, [_P]),
    ("jda_image_general_p1", C.c_uint32, [_P]),
    ("jda_output_geometry", C.c_int, [C.POINTER(ImageInfo), C.c_int32, C.c_int32] + [C.POINTER(C.c_int32)] * 5),
    ("jda_draw_plan", C.c_int, [C.POINTER(ImageInfo), C.c_int32, C.c_int32, C.c_int32, C.c_int32, _P, C.c_int32]),
    ("jda_crop_round", None, [C.POINTER(ImageInfo)] + [C.POINTER(C.c_int32)] * 4),
    ("jda_draw_plan_ex", C.c_int, [C.POINTER(ImageInfo), C.c_int32, C.c_int32, C.c_int32, C.c_int32, _P, _P, C.c_int32]),
    ("jda_draw_plan_at", C.c_int, [C.POINTER(ImageInfo), C.c_int32, C.c_int32, C.c_int32, C.c_int32, _P, C.c_int32, _P, C.c_int32]),
    ("jda_device_count", C.c_int, []),
    ("jda_create", _P, [C.c_int32, C.POINTER(C.c_int32)]),
    ("jda_destroy", None, [_P]),
    ("jda_last_hip_error", C.c_char_p, [_P]),
    ("jda_stream", _P, [_P]),
    ("jda_malloc", _P, [_P, C.c_size_t]),
    ("jda_free", None, [_P, _P]),
    ("jda_memset", C.c_int, [_P, _P, C.c_int, C.c_size_t]),
    ("jda_copy_to_host", C.c_int, [_P, _P, _P, C.c_size_t]),
    ("jda_copy_to_device", C.c_int, [_P, _P, _P, C.c_size_t]),
    ("jda_upload", _P, [_P, _P, C.POINTER(C.c_int32)]),
    ("jda_dev_image_free", None, [_P, _P]),
    ("jda_dev_image_bytes", C.c_size_t, [_P]),
    ("jda_batch_create", _P, [_P, C.c_int32, C.POINTER(_P), C.POINTER(Output), C.POINTER(C.c_int32),
                              C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    ("jda_batch_destroy", None, [_P, _P]),
    ("jda_batch_decode", C.c_int, [_P, _P]),
    ("jda_batch_get_stats", C.c_int, [_P, C.POINTER(BatchStats)]),
    ("jda_sync", C.c_int, [_P]),
    ("jda_timer_start", C.c_int, [_P]),
    ("jda_timer_stop", C.c_int, [_P]),
    ("jda_timer_elapsed_ms", C.c_double, [_P]),
    ("jda_decode_to_host", C.c_int, [_P, C.c_char_p, C.c_int32, C.c_int32, C.c_int32, _P, C.c_int32, C.c_int32]),
    ("jda_decode_to_host_ex", C.c_int, [_P, C.c_char_p, C.c_int32, C.c_int32, C.c_int32, _P, C.c_int32, C.c_int32, C.POINTER(C.c_int32)]),
    ("jda_pipeline_create", _P, [_P, C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.c_int32)]),
    ("jda_pipeline_destroy", None, [_P]),
    ("jda_pipeline_submit_ex", C.c_int, [_P, C.c_int32, C.POINTER(C.c_char_p), C.POINTER(C.c_int32), C.POINTER(Output), C.POINTER(C.c_int32),
                                         C.POINTER(C.c_int32), C.c_int32, C.POINTER(C.c_int32)]),
    ("jda_pipeline_submit", C.c_int, [_P, C.c_int32, C.POINTER(C.c_char_p), C.POINTER(C.c_int32), C.POINTER(Output), C.POINTER(C.c_int32),
                                      C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    ("jda_pipeline_wait", C.c_int, [_P, C.c_int32, C.POINTER(C.c_int32)]),
    ("jda_pipeline_get_stats", C.c_int, [_P, C.POINTER(PipelineStats)]),
    ("jda_pipeline_read_index", C.c_int, [_P, C.c_int32, C.c_int32, _P, _P, C.POINTER(C.c_uint32)]),
    ("jda_dither_geometry", C.c_int, [C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int64)]),
    ("jda_dither_seed", C.c_int, [C.c_char_p, C.c_int32, C.c_int32, _P]),
    ("jda_dither_surfaces", C.c_int, [_P, C.c_int32, C.POINTER(Output), C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(_P), C.POINTER(Output)]),
    ("jda_decode_dither_to_host", C.c_int, [_P, C.c_char_p, C.c_int32, C.c_int32, C.c_int32, _P, _P, C.c_int32, C.c_int32, C.POINTER(C.c_int32)]),
    ("jda_oriented_geometry", C.c_int, [C.POINTER(ImageInfo), C.c_int32, C.c_int32, C.c_int32] + [C.POINTER(C.c_int32)] * 4),
    ("jda_orient_surfaces", C.c_int, [_P, C.c_int32, C.POINTER(Output), C.c_int32, C.POINTER(C.c_int32), C.POINTER(Output)]),
    ("jda_decode_to_host_oriented", C.c_int, [_P, C.c_char_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, _P, C.c_int32, C.c_int32, C.POINTER(C.c_int32)]),
    ("jda_pack_bytes", C.c_size_t, [C.c_int32] * 4),
    ("jda_pack_surfaces", C.c_int, [_P, C.c_int32, C.POINTER(Output), C.c_int32, C.POINTER(C.c_int32), C.c_int32, C.c_int32, _P, C.POINTER(_P)]),
    ("jda_unpack_surfaces", C.c_int, [_P, C.c_int32, C.POINTER(_P), C.c_int32, C.c_int32, C.POINTER(C.c_float), C.POINTER(Output), C.c_int32]),
    ("jda_encode_dense_to_host", C.c_int, [_P, _P] + [C.c_int32] * 5 + [C.POINTER(C.c_float)] + [C.c_int32] * 4 + [_P, C.c_int64, C.POINTER(C.c_int64)]),
    ("jda_decode_to_host_packed", C.c_int, [_P, C.c_char_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, _P, _P, C.c_size_t] + [C.POINTER(C.c_int32)] * 3),
    ("jda_resize_surfaces", C.c_int, [_P, C.c_int32, C.POINTER(Output), C.c_int32, C.POINTER(C.c_int32), C.POINTER(Output)]),
    ("jda_resize_surfaces_ex", C.c_int, [_P, C.c_int32, C.POINTER(Output), C.c_int32, C.POINTER(C.c_int32), C.POINTER(Output), C.c_int32]),
    ("jda_resize_surfaces_box", C.c_int, [_P, C.c_int32, C.POINTER(Output), C.c_int32, C.POINTER(C.c_float), C.POINTER(Output), C.c_int32]),
    ("jda_reduce_geometry", C.c_int, [C.c_int32] * 4 + [C.POINTER(C.c_int32)] * 2),
    ("jda_reduce_surfaces", C.c_int, [_P, C.c_int32, C.POINTER(Output), C.c_int32, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(Output)]),
    ("jda_thumbnail_plan", C.c_int, [C.c_int32] * 5 + [C.c_double, C.POINTER(ThumbnailSteps)]),
    ("jda_decode_to_host_thumbnail", C.c_int, [_P, C.c_char_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_double, C.c_int32, _P, C.c_int32, C.c_int32,
                                               C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    ("jda_transcode_to_host", C.c_int, [_P, C.c_char_p, C.c_int32, C.c_int32, C.POINTER(C.c_int32), C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, _P,
                                        C.c_int64, C.POINTER(C.c_int64)]),
    ("jda_transcode_to_host_ex", C.c_int, [_P, C.c_char_p, C.c_int32, C.c_int32, C.POINTER(C.c_int32), C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_uint32,
                                           _P, C.c_int64, C.POINTER(C.c_int64)]),
    ("jda_encode_bound", C.c_int, [C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.c_int64)]),
    ("jda_encode_surfaces_ex", C.c_int, [_P, C.c_int32, C.POINTER(Output), C.c_int32, C.POINTER(EncodeJob), C.POINTER(C.c_uint32), C.POINTER(C.c_void_p),
                                         C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(C.c_int32)]),
    ("jda_encode_bound_progressive", C.c_int, [C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.c_int64)]),
    ("jda_encode_surfaces_progressive", C.c_int, [_P, C.c_int32, C.POINTER(Output), C.c_int32, C.POINTER(EncodeJob), C.POINTER(C.c_void_p), C.POINTER(C.c_int64),
                                                  C.POINTER(C.c_int64), C.POINTER(C.c_int32)]),
    ("jda_transcode_to_host_progressive", C.c_int, [_P, C.c_char_p, C.c_int32, C.c_int32, C.POINTER(C.c_int32), C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, _P,
                                                    C.c_int64, C.POINTER(C.c_int64)]),
    ("jda_encode_surfaces", C.c_int, [_P, C.c_int32, C.POINTER(Output), C.c_int32, C.POINTER(EncodeJob), C.POINTER(C.c_void_p), C.POINTER(C.c_int64),
                                      C.POINTER(C.c_int64), C.POINTER(C.c_int32)]),
    ("jda_decode_to_host_resized", C.c_int, [_P, C.c_char_p] + [C.c_int32] * 3 + [C.POINTER(C.c_int32), C.c_int32, C.c_int32, _P, C.c_int32, C.c_int32, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    ("jda_decode_to_host_resized_ex", C.c_int, [_P, C.c_char_p] + [C.c_int32] * 3 + [C.POINTER(C.c_int32), C.c_int32, C.c_int32, C.c_int32, _P, C.c_int32, C.c_int32, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    ("jda_checksum_surfaces", C.c_int, [_P, C.c_int32, C.POINTER(Output), C.POINTER(C.c_int32), C.POINTER(C.c_uint64)]),
    ("jda_device_pci_bus_id", C.c_int, [_P, C.c_char_p, C.c_int32]),
    ("jda_upload_batch_ex", C.c_int, [_P, C.c_int32, C.POINTER(_P), C.POINTER(_P), C.POINTER(C.c_int32)]),
    ("jda_batch_get_status", C.c_int, [_P, C.POINTER(C.c_int32)]),
    ("jda_decode_to_host_rect", C.c_int, [_P, C.c_char_p, C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.c_int32), _P, C.c_int32, C.c_int32,
                                          C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    ("jda_batch_create_rect", _P, [_P, C.c_int32, C.POINTER(_P), C.POINTER(Output), C.POINTER(C.c_int32), C.POINTER(C.c_int32),
                                   C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    ("jda_version", C.c_char_p, []),
    ("jda_host_alloc", _P, [C.c_size_t]),
    ("jda_host_free", None, [_P]),
    ("jda_host_register", C.c_int, [_P, C.c_size_t]),
    ("jda_host_unregister", C.c_int, [_P]),
    ("jda_progressive_full_requested", C.c_int, [C.POINTER(ImageInfo), C.c_int32]),
    ("jda_progressive_prepare", _P, [C.c_char_p, C.c_int32, C.POINTER(C.c_int32)]),
    ("jda_coef_image_from_coefficients", _P, [C.c_char_p, C.c_int32, _P, C.c_uint32, C.POINTER(C.c_int32)]),
    ("jda_coef_image_free", None, [_P]),
    ("jda_coef_image_get_info", C.POINTER(ImageInfo), [_P]),
    ("jda_coef_image_coefficients", _P, [_P, C.POINTER(C.c_uint32)]),
    ("jda_coef_image_quant", _P, [_P, _P]),
    ("jda_coef_image_sparse", _P, [_P, C.POINTER(_P), C.POINTER(C.c_uint32)]),
    ("jda_coef_image_sparse_status", C.c_int, [_P]),
    ("jda_coef_image_sparse_bytes", C.c_size_t, [_P]),
    ("jda_coef_upload", _P, [_P, _P, C.POINTER(C.c_int32)]),
    ("jda_coef_upload_ex", _P, [_P, _P, C.c_int32, C.POINTER(C.c_int32)]),
    ("jda_dev_coef_form", C.c_int, [_P]),
    ("jda_dev_coef_bytes", C.c_size_t, [_P]),
    ("jda_coef_decode_surfaces_rect", C.c_int, [_P, C.c_int32, C.POINTER(_P), C.POINTER(Output), C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    ("jda_dev_coef_free", None, [_P, _P]),
    ("jda_coef_decode_surfaces", C.c_int, [_P, C.c_int32, C.POINTER(_P), C.POINTER(Output), C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    ("jda_recode_bound", C.c_int, [C.POINTER(ImageInfo), C.c_int32, C.c_int32, C.POINTER(C.c_int64)]),
    ("jda_recode_images", C.c_int, [_P, C.c_int32, C.POINTER(RecodeSource), C.POINTER(RecodeJob), C.POINTER(C.c_void_p), C.POINTER(C.c_int64), C.POINTER(C.c_int64),
                                    C.POINTER(C.c_int32)]),
    ("jda_recode_to_host", C.c_int, [_P, C.c_char_p, C.c_int32, C.c_int32, C.c_int32, _P, C.c_int64, C.POINTER(C.c_int64)]),
    ("jda_recode_geometry", C.c_int, [C.POINTER(ImageInfo), C.POINTER(RecodeXform), C.POINTER(ImageInfo)]),
    ("jda_recode_bound_ex", C.c_int, [C.POINTER(ImageInfo), C.POINTER(RecodeXform), C.c_int32, C.c_int32, C.POINTER(C.c_int64)]),
    ("jda_recode_images_ex", C.c_int, [_P, C.c_int32, C.POINTER(RecodeSource), C.POINTER(RecodeJob), C.POINTER(RecodeXform), C.POINTER(C.c_void_p), C.POINTER(C.c_int64),
                                       C.POINTER(C.c_int64), C.POINTER(C.c_int32)]),
    ("jda_recode_to_host_ex", C.c_int, [_P, C.c_char_p, C.c_int32, C.c_int32, C.c_int32, C.POINTER(RecodeXform), _P, C.c_int64, C.POINTER(C.c_int64)]),
    ("jda_exact_decode_surfaces", C.c_int, [_P, C.c_int32, C.POINTER(RecodeSource), C.POINTER(Output), C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    ("jda_exact_decode_planes", C.c_int, [_P, C.c_int32, C.POINTER(RecodeSource), C.POINTER(Output), C.POINTER(C.c_int32)]),
    ("jda_decode_to_host_exact", C.c_int, [_P, C.c_char_p, C.c_int32, C.c_int32, _P, C.c_int32, C.c_int32]),
    ("jda_exact_scaled_geometry", C.c_int, [C.POINTER(ImageInfo), C.c_int32, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    ("jda_exact_draft_scale", C.c_int, [C.POINTER(ImageInfo), C.c_int32, C.c_int32]),
    ("jda_exact_decode_surfaces_scaled", C.c_int, [_P, C.c_int32, C.POINTER(RecodeSource), C.POINTER(Output), C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    ("jda_exact_decode_planes_scaled", C.c_int, [_P, C.c_int32, C.POINTER(RecodeSource), C.POINTER(Output), C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    ("jda_decode_to_host_exact_scaled", C.c_int, [_P, C.c_char_p, C.c_int32, C.c_int32, C.c_int32, _P, C.c_int32, C.c_int32]),
    ("jda_exact_probe", C.c_int, [C.c_char_p, C.c_int32, _P]),
    ("jda_coef_prepare", _P, [C.c_char_p, C.c_int32, C.POINTER(C.c_int32)]),
    ("jda_coef_image_component3", _P, [_P]),
    ("jda_exact_decode_surfaces_ex", C.c_int, [_P, C.c_int32, C.POINTER(RecodeSource), C.POINTER(Output), C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.c_uint32, C.POINTER(C.c_int32)]),
    ("jda_exact_decode_planes_ex", C.c_int, [_P, C.c_int32, C.POINTER(RecodeSource), C.POINTER(Output), C.POINTER(C.c_int32), C.c_uint32, C.POINTER(C.c_int32)]),
    ("jda_decode_to_host_exact_ex", C.c_int, [_P, C.c_char_p, C.c_int32, C.c_int32, C.c_int32, C.c_uint32, _P, C.c_int32, C.c_int32]),
    ("jda_exact_decode_surfaces_rect", C.c_int, [_P, C.c_int32, C.POINTER(RecodeSource), C.POINTER(Output), C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.c_uint32,
                                                 C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    ("jda_exact_rect_mcus", C.c_int, [C.POINTER(ImageInfo), C.c_int32, C.c_int32, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    ("jda_decode_to_host_exact_rect", C.c_int, [_P, C.c_char_p, C.c_int32, C.c_int32, C.c_int32, C.c_uint32, C.POINTER(C.c_int32), _P, C.c_int32, C.c_int32, C.POINTER(C.c_int32)]),
    ("jda_resize_reads", C.c_int, [C.c_int32, C.c_int32, C.POINTER(C.c_int32), C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.c_int32)]),
]


def load_library():
    """Load libjpegdec_amd.so (built by `make lib` / __graft_entry__.build()).  Raises if absent."""
    global _lib
    if _lib is not None:
        return _lib
    path = library_path()
    if not os.path.exists(path):
        raise FileNotFoundError("%s is missing: build it with `make lib` (hipcc --offload-arch=gfx950); "
                                "jpegdec_amd has no CPU fallback" % path)
    lib = C.CDLL(path)
    for name, res, args in _PROTOTYPES:
        fn = getattr(lib, name)   # AttributeError if the library does not export a declared symbol
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


def parse(jpeg: bytes) -> dict:
    info = ImageInfo()
    rc = load_library().jda_parse(jpeg, len(jpeg), C.byref(info))
    d = info.as_dict()
    d["status"] = rc
    return d


def output_geometry(info: ImageInfo, pixel_type=RGB8888, options=0):
    vals = [C.c_int32(0) for _ in range(5)]
    rc = load_library().jda_output_geometry(C.byref(info), pixel_type, options, *[C.byref(v) for v in vals])
    if rc != 0:
        raise JdaError(rc, "jda_output_geometry")
    return dict(zip(("bpp", "out_w", "out_h", "canvas_w", "canvas_h"), [v.value for v in vals]))


def draw_plan(info: ImageInfo, pixel_type=RGB8888, options=0, max_mcus=0, uses_dma=False):
    rects = np.zeros((1 << 16, 6), dtype=np.int32)
    n = load_library().jda_draw_plan(C.byref(info), pixel_type, options, max_mcus, 1 if uses_dma else 0,
                                     rects.ctypes.data_as(_P), rects.shape[0])
    return rects[: max(n, 0)].copy()


def crop_round(info: ImageInfo, x, y, w, h):
    v = [C.c_int32(a) for a in (x, y, w, h)]
    load_library().jda_crop_round(C.byref(info), *[C.byref(a) for a in v])
    return tuple(a.value for a in v)


def draw_plan_ex(info: ImageInfo, pixel_type=RGB8888, options=0, max_mcus=0, uses_dma=False, crop=None):
    rects = np.zeros((1 << 16, 8), dtype=np.int32)
    carr = (C.c_int32 * 4)(*crop) if crop is not None else None
    n = load_library().jda_draw_plan_ex(C.byref(info), pixel_type, options, max_mcus, 1 if uses_dma else 0,
                                        carr, rects.ctypes.data_as(_P), rects.shape[0])
    return rects[: max(n, 0)].copy()


PREPARE_DEVICE_PRESCAN = 1
PREPARE_CONT_ALWAYS = 2
PREPARE_CONT_NEVER = 4
PREPARE_SERIAL_PRESCAN = 8
PREPARE_PARALLEL_PRESCAN = 16


class PreparedImage:
    """Host-side result of parse + LUT build + scan filter + serial pre-scan (jda_prepare).

    device_prescan=True (jda_prepare_ex, JDA_PREPARE_DEVICE_PRESCAN): for a stream with restart markers the
    serial pre-scan is left to the GPU (done by DeviceImage / jda_upload); `prescan_pending` tells."""

    def __init__(self, jpeg: bytes, device_prescan: bool = False, _handle=None, flags: int = 0):
        """flags: further JDA_PREPARE_* bits (PREPARE_CONT_ALWAYS / PREPARE_CONT_NEVER)"""
        self.lib = load_library()
        err = C.c_int32(0)
        self.handle = _handle if _handle else self.lib.jda_prepare_ex(jpeg, len(jpeg), (PREPARE_DEVICE_PRESCAN if device_prescan else 0) | flags, C.byref(err))
        if not self.handle:
            raise JdaError(err.value, "jda_prepare")
        self.info = self.lib.jda_image_get_info(self.handle).contents

    def close(self):
        if self.handle:
            self.lib.jda_image_free(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def n_mcus(self):
        return self.info.mcus_x * self.info.mcus_y

    @property
    def prescan_pending(self) -> bool:
        return bool(self.lib.jda_image_prescan_pending(self.handle))

    def scan(self) -> np.ndarray:
        n = C.c_uint32(0)
        p = self.lib.jda_image_scan(self.handle, C.byref(n))
        return np.ctypeslib.as_array(C.cast(p, C.POINTER(C.c_uint8)), shape=(n.value,)).copy()

    @property
    def n_blocks(self):
        return self.n_mcus * self.info.blocks_per_mcu

    def block_index(self):
        """(index[n_blocks+1] uint32 = pos<<7|off per block, n_mcus_ok)"""
        n = C.c_uint32(0)
        p = self.lib.jda_image_block_index(self.handle, C.byref(n))
        arr = np.ctypeslib.as_array(C.cast(p, C.POINTER(C.c_uint32)), shape=(self.n_blocks + 1,)).copy()
        return arr, n.value

    def block_cont(self):
        """(cont_first[n_blocks + 1], cont[n]) -- the serial pre-scan's continuation entries (jda_image_block_cont)"""
        cf, n = _P(), C.c_uint32(0)
        p = self.lib.jda_image_block_cont(self.handle, C.byref(cf), C.byref(n))
        first = np.ctypeslib.as_array(C.cast(cf, C.POINTER(C.c_uint32)), shape=(self.n_blocks + 1,)).copy()
        ent = np.ctypeslib.as_array(C.cast(p, C.POINTER(C.c_uint32)), shape=(n.value,)).copy() if n.value else np.zeros(0, np.uint32)
        return first, ent

    def block_dc(self) -> np.ndarray:
        p = self.lib.jda_image_block_dc(self.handle)
        return np.ctypeslib.as_array(C.cast(p, C.POINTER(C.c_int16)), shape=(self.n_blocks,)).copy()

    def tables(self) -> np.ndarray:
        n = C.c_uint32(0)
        p = self.lib.jda_image_tables(self.handle, C.byref(n))
        return np.ctypeslib.as_array(C.cast(p, C.POINTER(C.c_uint8)), shape=(n.value,)).copy()

    def truncation_events(self) -> int:
        return self.lib.jda_image_truncation_events(self.handle)

    def general_p1(self) -> bool:
        """An AC table codes EOB twice: the kernels cannot find EOB by one compare and take their general bit reader."""
        return bool(self.lib.jda_image_general_p1(self.handle))

    def geometry(self, pixel_type=RGB8888, options=0):
        return output_geometry(self.info, pixel_type, options)


class Context:
    """One per process per GPU: HIP device + stream + timing events (jda_create)."""

    def __init__(self, device: int = 0):
        self.lib = load_library()
        err = C.c_int32(0)
        self.handle = self.lib.jda_create(device, C.byref(err))
        if not self.handle:
            raise JdaError(err.value, "jda_create(device=%d): no usable HIP device -- there is no CPU fallback" % device)
        self.device = device

    def close(self):
        if self.handle:
            self.lib.jda_destroy(self.handle)
            self.handle = None

    def check(self, rc, what=""):
        if rc != 0:
            raise JdaError(rc, what + ": " + (self.lib.jda_last_hip_error(self.handle) or b"").decode())

    def malloc(self, nbytes: int) -> int:
        p = self.lib.jda_malloc(self.handle, nbytes)
        if not p:
            raise JdaError(5, "jda_malloc(%d)" % nbytes)
        return p

    def free(self, ptr):
        self.lib.jda_free(self.handle, ptr)

    def memset(self, ptr, value, nbytes):
        self.check(self.lib.jda_memset(self.handle, ptr, value, nbytes), "jda_memset")

    def to_host(self, ptr, nbytes) -> np.ndarray:
        out = np.empty(nbytes, dtype=np.uint8)
        self.check(self.lib.jda_copy_to_host(self.handle, out.ctypes.data_as(_P), ptr, nbytes), "jda_copy_to_host")
        return out

    def sync(self):
        self.check(self.lib.jda_sync(self.handle), "jda_sync")

    def checksums(self, surfaces, row_bytes):
        """jda_checksum_surfaces: surfaces = list of (device_ptr, pitch_bytes, width_px, rows); one uint64 per surface."""
        n = len(surfaces)
        outs = (Output * n)(*[Output(*o) for o in surfaces])
        rb = (C.c_int32 * n)(*row_bytes)
        res = (C.c_uint64 * n)()
        self.check(self.lib.jda_checksum_surfaces(self.handle, n, outs, rb, res), "jda_checksum_surfaces")
        return [int(v) for v in res]

    def from_host(self, ptr, data):
        a = np.ascontiguousarray(data, dtype=np.uint8)
        self.check(self.lib.jda_copy_to_device(self.handle, ptr, a.ctypes.data_as(_P), a.size), "jda_copy_to_device")

    def pci_bus_id(self) -> str:
        buf = C.create_string_buffer(32)
        self.check(self.lib.jda_device_pci_bus_id(self.handle, buf, 32), "jda_device_pci_bus_id")
        return buf.value.decode()

    def timer_start(self):
        self.check(self.lib.jda_timer_start(self.handle), "jda_timer_start")

    def timer_stop(self):
        self.check(self.lib.jda_timer_stop(self.handle), "jda_timer_stop")

    def timer_elapsed_ms(self) -> float:
        return self.lib.jda_timer_elapsed_ms(self.handle)


class DeviceImage:
    """Inputs of one image resident in HBM (jda_upload)."""

    def __init__(self, ctx: Context, prepared: PreparedImage, _handle=None):
        self.ctx = ctx
        err = C.c_int32(0)
        self.handle = _handle if _handle else ctx.lib.jda_upload(ctx.handle, prepared.handle, C.byref(err))
        if not self.handle:
            raise JdaError(err.value, "jda_upload")
        self.info = ImageInfo.from_buffer_copy(prepared.info)
        self.nbytes = ctx.lib.jda_dev_image_bytes(self.handle)
        self.prescan_on_device = bool(ctx.lib.jda_dev_image_prescan_on_device(self.handle))
        self.n_mcus_ok = int(ctx.lib.jda_dev_image_mcus_ok(self.handle))

    def read_index(self):
        """(index[n_blocks + 1] uint32, dc[n_blocks] int16) as they stand in HBM"""
        nb = self.info.mcus_x * self.info.mcus_y * self.info.blocks_per_mcu
        idx = np.zeros(nb + 1, np.uint32)
        dc = np.zeros(nb, np.int16)
        rc = self.ctx.lib.jda_dev_image_read_index(self.ctx.handle, self.handle, idx.ctypes.data_as(C.c_void_p), dc.ctypes.data_as(C.c_void_p))
        if rc != 0:
            raise JdaError(rc, "jda_dev_image_read_index")
        return idx, dc

    def close(self):
        if self.handle:
            self.ctx.lib.jda_dev_image_free(self.ctx.handle, self.handle)
            self.handle = None


def index_equivalent(a, b) -> bool:
    """Do two per-block indexes (format 2) name the same decode?  An entry is (byte position << 7) | flag << 6 | bit offset: the
    bit position pos * 8 + off of the block's FIRST AC SYMBOL is what P1 starts from; the split into (pos, off) -- the reference
    reader's phase behind the refill at the top of its AC loop -- only matters for a block flagged JDA_INDEX_TRUNC (its truncated
    magnitude reads are emulated from that phase).  The serial pre-scan writes the true phase everywhere, the device pre-scan a
    canonical one ((p >> 3) << 7 | p & 7) into unflagged entries: equivalent = same bit position and flag in every block's entry,
    same entry where flagged.  The closing entry (the last one) only bounds the scan from above: the device pre-scan's lies up to
    41 bits behind the serial one's (the DC symbol the stream's padding decodes to, an interval's rounding); either order of
    the arguments is accepted."""
    a = np.ascontiguousarray(a, dtype=np.uint32)
    b = np.ascontiguousarray(b, dtype=np.uint32)
    if a.shape != b.shape or a.ndim != 1 or a.size == 0:
        return False
    return bool(load_library().jda_index_equivalent(a.ctypes.data_as(C.c_void_p), b.ctypes.data_as(C.c_void_p), a.size - 1))


def prepare_batch(jpegs, device_prescan: bool = False, threads: int = 0, strict: bool = True, flags: int = 0):
    """jda_prepare_batch: the images are prepared on `threads` host threads (0 = all).  strict=False: a rejected file leaves a
    None in the list (and its error code in the second return value) instead of failing the whole batch."""
    lib = load_library()
    n = len(jpegs)
    arr = (C.c_char_p * n)(*jpegs)
    lens = (C.c_int32 * n)(*[len(j) for j in jpegs])
    outs = (_P * n)()
    errs = (C.c_int32 * n)()
    rc = lib.jda_prepare_batch(n, arr, lens, (PREPARE_DEVICE_PRESCAN if device_prescan else 0) | flags, threads, outs, errs)
    res = [PreparedImage(jpegs[i], _handle=outs[i]) if outs[i] else None for i in range(n)]
    if not strict:
        return res, list(errs)
    if rc != 0:
        for r in res:
            if r is not None:
                r.close()
        raise JdaError(rc, "jda_prepare_batch")
    return res


def upload_batch(ctx: Context, prepared_list):
    """jda_upload_batch: all images in one go (pending block indexes are made on the GPU in two launches)."""
    n = len(prepared_list)
    himgs = (_P * n)(*[(p.handle if p is not None else None) for p in prepared_list])
    outs = (_P * n)()
    st = (C.c_int32 * n)()
    rc = ctx.lib.jda_upload_batch_ex(ctx.handle, n, himgs, outs, st)      # holes (None) stay holes
    if rc != 0:
        raise JdaError(rc, "jda_upload_batch")
    return [DeviceImage(ctx, prepared_list[i], _handle=outs[i]) if outs[i] else None for i in range(n)]


class Batch:
    """Launch plan over resident images (jda_batch_create / jda_batch_decode)."""

    def __init__(self, ctx: Context, images, outputs, pixel_types, options, mcu_rects=None):
        """outputs: list of (device_ptr, pitch_bytes, width_px, rows).  mcu_rects: None, or one (mx0, my0, mx1, my1) per image
        (jda_batch_create_rect; an image's entry is ignored where the image is a hole and may be None there)."""
        n = len(images)
        self.ctx = ctx
        self.n = n
        himgs = (_P * n)(*[(im.handle if im is not None else None) for im in images])
        outs = (Output * n)(*[Output(*o) for o in outputs])
        pts = (C.c_int32 * n)(*pixel_types)
        opts = (C.c_int32 * n)(*options)
        err = C.c_int32(0)
        if mcu_rects is None:
            self.handle = ctx.lib.jda_batch_create(ctx.handle, n, himgs, outs, pts, opts, C.byref(err))
        else:
            if len(mcu_rects) != n or any(r is None and im is not None for r, im in zip(mcu_rects, images)):
                raise ValueError("mcu_rects: one rectangle per image")
            rects = (C.c_int32 * (4 * n))(*[v for r in mcu_rects for v in (r if r is not None else (0, 0, 0, 0))])
            self.handle = ctx.lib.jda_batch_create_rect(ctx.handle, n, himgs, outs, pts, opts, rects, C.byref(err))
        if not self.handle:
            raise JdaError(err.value, "jda_batch_create: " + (ctx.lib.jda_last_hip_error(ctx.handle) or b"").decode())
        st = BatchStats()
        ctx.lib.jda_batch_get_stats(self.handle, C.byref(st))
        self.stats = {k: getattr(st, k) for k, _ in BatchStats._fields_}

    def decode(self):
        self.ctx.check(self.ctx.lib.jda_batch_decode(self.ctx.handle, self.handle), "jda_batch_decode")

    def status(self):
        """per image: 0, 2 (JDA_DECODE_ERROR: bad MCU, the MCUs before it are decoded) or 1 (a hole in the image list)"""
        st = (C.c_int32 * self.n)()
        self.ctx.check(self.ctx.lib.jda_batch_get_status(self.handle, st), "jda_batch_get_status")
        return list(st)

    def close(self):
        if self.handle:
            self.ctx.lib.jda_batch_destroy(self.ctx.handle, self.handle)
            self.handle = None


class Pipeline:
    """The streamed pipeline (jda_pipeline_*): files in, pixels resident in HBM out; upload + filter + pre-scan of the next
    batch run under the decode of the current one."""

    def __init__(self, ctx: Context, max_images: int, depth: int = 2, host_threads: int = 0):
        self.ctx = ctx
        err = C.c_int32(0)
        self.handle = ctx.lib.jda_pipeline_create(ctx.handle, max_images, depth, host_threads, C.byref(err))
        if not self.handle:
            raise JdaError(err.value, "jda_pipeline_create")
        self._keep = {}

    @staticmethod
    def pack(jpegs, outputs, pixel_types, options):
        """The C arrays of one submit (a caller that streams the same list again and again builds them once: a C caller has them
        anyway, and per image they cost Python as much as the GPU takes for a 1280x720 file)."""
        n = len(jpegs)
        arr = (C.c_char_p * n)(*jpegs)
        lens = (C.c_int32 * n)(*[len(j) for j in jpegs])
        outs = (Output * n)(*[Output(*o) for o in outputs])
        pts = (C.c_int32 * n)(*pixel_types)
        opts = (C.c_int32 * n)(*options)
        return (jpegs, arr, lens, outs, pts, opts, n)

    @staticmethod
    def pack_pinned(pinned, picks, outputs, pixel_types, options):
        """The same for files that lie in page-locked memory (PinnedFiles): picks = indices into it.  Submitted with
        JDA_SUBMIT_PINNED_INPUT, the copy engine reads them where they are."""
        n = len(picks)
        arr = (C.c_void_p * n)(*[pinned.addrs[k] for k in picks])
        lens = (C.c_int32 * n)(*[pinned.lens[k] for k in picks])
        outs = (Output * n)(*[Output(*o) for o in outputs])
        pts = (C.c_int32 * n)(*pixel_types)
        opts = (C.c_int32 * n)(*options)
        return (pinned, C.cast(arr, C.POINTER(C.c_char_p)), lens, outs, pts, opts, n, arr)

    def submit_packed(self, packed, flags: int = 0) -> int:
        arr, lens, outs, pts, opts, n = packed[1:7]
        t = C.c_int32(-1)
        self.ctx.check(self.ctx.lib.jda_pipeline_submit_ex(self.handle, n, arr, lens, outs, pts, opts, flags, C.byref(t)), "jda_pipeline_submit_ex")
        self._keep[t.value] = packed                                      # the buffers stay alive until the batch is waited for
        return t.value

    def submit(self, jpegs, outputs, pixel_types, options, flags: int = 0) -> int:
        """outputs: list of (device_ptr, pitch_bytes, width_px, rows).  flags: SUBMIT_* bits (SUBMIT_PROGRESSIVE_FULL: a progressive file
        whose option word carries PROGRESSIVE_FULL is decoded at full size instead of refused).  Returns the batch's ticket."""
        return self.submit_packed(self.pack(jpegs, outputs, pixel_types, options), flags)

    def wait(self, ticket: int):
        """Blocks until the batch is decoded; returns the list of per-image status codes."""
        n = self._keep[ticket][6]
        st = (C.c_int32 * n)()
        self.ctx.check(self.ctx.lib.jda_pipeline_wait(self.handle, ticket, st), "jda_pipeline_wait")
        del self._keep[ticket]
        return list(st)

    def read_index(self, ticket: int, i: int, n_blocks: int):
        idx = np.zeros(n_blocks + 1, np.uint32)
        dc = np.zeros(n_blocks, np.int16)
        flen = C.c_uint32(0)
        rc = self.ctx.lib.jda_pipeline_read_index(self.handle, ticket, i, idx.ctypes.data_as(_P), dc.ctypes.data_as(_P), C.byref(flen))
        if rc != 0:
            raise JdaError(rc, "jda_pipeline_read_index")
        return idx, dc, flen.value

    @property
    def stats(self):
        st = PipelineStats()
        self.ctx.lib.jda_pipeline_get_stats(self.handle, C.byref(st))
        return {k: getattr(st, k) for k, _ in PipelineStats._fields_}

    def close(self):
        if self.handle:
            self.ctx.lib.jda_pipeline_destroy(self.handle)
            self.handle = None


class PinnedFiles:
    """Files copied once into page-locked host memory: what a loader that reads into page-locked memory hands to
    jda_pipeline_submit_ex(.., JDA_SUBMIT_PINNED_INPUT, ..).  Default: ONE arena (jda_host_alloc), each file at a 4 KB boundary.
    separate=True: one allocation of exactly the file's size per file, alternately jda_host_alloc and a malloc'ed buffer made
    known with jda_host_register (separate page-locked objects: no copy may run over the end of one or across two)."""

    def __init__(self, files, separate: bool = False):
        self.lib = load_library()
        self.lens = [len(f) for f in files]
        self.base, self._allocs, self._registered = None, [], []
        if separate:
            self.addrs = []
            for k, f in enumerate(files):
                if k & 1:
                    buf = C.create_string_buffer(len(f))
                    if self.lib.jda_host_register(C.addressof(buf), len(f)) != 0:
                        raise JdaError(5, "jda_host_register(%d)" % len(f))
                    self._registered.append(buf)
                    a = C.addressof(buf)
                else:
                    a = self.lib.jda_host_alloc(len(f))
                    if not a:
                        raise JdaError(5, "jda_host_alloc(%d)" % len(f))
                    self._allocs.append(a)
                C.memmove(a, f, len(f))
                self.addrs.append(a)
            self.bytes = sum(self.lens)
            return
        offs, total = [], 0
        for ln in self.lens:
            offs.append(total)
            total += (ln + 4095) & ~4095
        self.bytes = total
        self.base = self.lib.jda_host_alloc(max(total, 4096))
        if not self.base:
            raise JdaError(5, "jda_host_alloc(%d)" % total)
        self.addrs = [self.base + o for o in offs]
        for a, f in zip(self.addrs, files):
            C.memmove(a, f, len(f))

    def close(self):
        if self.base:
            self.lib.jda_host_free(self.base)
            self.base = None
        for a in self._allocs:
            self.lib.jda_host_free(a)
        for buf in self._registered:
            self.lib.jda_host_unregister(C.addressof(buf))
        self._allocs, self._registered = [], []


SUBMIT_PINNED_INPUT = 1
SUBMIT_PROGRESSIVE_FULL = 2      # honour PROGRESSIVE_FULL in a progressive file's option word (without it: status 3, as ever)
COEF_DENSE, COEF_SPARSE, COEF_AUTO = 0, 1, 2      # jda_coef_upload_ex: the form that travels (AUTO: the smaller one for the image)


def surface_checksum_host(canvas: np.ndarray) -> int:
    """The same checksum as Context.checksums, of a host array (rows x row_bytes uint8): the reference value in tests."""
    rows, row_bytes = canvas.shape
    dpr = (row_bytes + 3) // 4
    pad = np.zeros((rows, dpr * 4), np.uint8)
    pad[:, :row_bytes] = canvas
    d = pad.view("<u4").reshape(-1).astype(np.uint64)
    i = np.arange(d.size, dtype=np.uint64)
    m = ((d ^ ((i * np.uint64(0x9E3779B1)) & np.uint64(0xFFFFFFFF))) * np.uint64(0x85EBCA6B)) & np.uint64(0xFFFFFFFF)
    with np.errstate(over="ignore"):
        return int(np.sum(m * (np.uint64(2) * i + np.uint64(1)), dtype=np.uint64))


def decode_to_host(ctx: Context, jpeg: bytes, pixel_type=RGB8888, options=0, out=None):
    """Decode one image through the GPU path into an MCU-padded host canvas (rows x pitch bytes).
    out: a canvas of that shape from an earlier call, to decode into (a fresh 4096x4096 canvas costs a millisecond of page faults)."""
    info = ImageInfo()
    rc = ctx.lib.jda_parse(jpeg, len(jpeg), C.byref(info))
    if rc != 0:
        raise JdaError(rc, "jda_parse")
    g = output_geometry(info, pixel_type, options)
    shape = (g["canvas_h"], g["canvas_w"] * g["bpp"])
    canvas = out if out is not None and out.shape == shape and out.dtype == np.uint8 and out.flags["C_CONTIGUOUS"] else np.zeros(shape, dtype=np.uint8)
    rc = ctx.lib.jda_decode_to_host(ctx.handle, jpeg, len(jpeg), pixel_type, options,
                                    canvas.ctypes.data_as(_P), canvas.shape[1], canvas.shape[0])
    return rc, canvas, g


class CoefImage:
    """A coefficient image (host): every scan of a progressive file decoded by jda_progressive_prepare, or -- coefs given -- the
    caller's own coefficients under the headers of any supported file (jda_coef_image_from_coefficients).  coefs: int16,
    (blocks, 64), natural order, blocks in MCU-interleaved scan order."""
    def __init__(self, jpeg: bytes, coefs=None, any_file=False):
        self.lib = load_library()
        self.owned = True
        err = C.c_int32(0)
        if any_file:
            self.handle = self.lib.jda_coef_prepare(jpeg, len(jpeg), C.byref(err))
        elif coefs is None:
            self.handle = self.lib.jda_progressive_prepare(jpeg, len(jpeg), C.byref(err))
        else:
            a = np.ascontiguousarray(coefs, dtype=np.int16).reshape(-1, 64)
            self.handle = self.lib.jda_coef_image_from_coefficients(jpeg, len(jpeg), a.ctypes.data_as(_P), a.shape[0], C.byref(err))
        if not self.handle:
            raise JdaError(err.value, "jda_coef_prepare" if any_file else "jda_progressive_prepare" if coefs is None else "jda_coef_image_from_coefficients")
        self.info = self.lib.jda_coef_image_get_info(self.handle).contents

    @classmethod
    def from_file(cls, jpeg: bytes):
        """jda_coef_prepare: every scan of a Huffman-coded 8-bit file of one, three or four components, sequential or progressive.  A
        four-component image holds components 0..2 as a three-component image (coefficients(), info.ncomp == 4) and component 3 as
        component3(), a gray image; only the exact decode with colour_models=True takes it."""
        return cls(jpeg, any_file=True)

    def component3(self):
        """component 3 of a four-component image as the gray coefficient image it is stored as (a view: it lives as long as this one), or None"""
        h = self.lib.jda_coef_image_component3(self.handle)
        if not h:
            return None
        k = object.__new__(CoefImage)
        k.lib, k.handle, k.owned, k.parent = self.lib, h, False, self
        k.info = self.lib.jda_coef_image_get_info(h).contents
        return k

    def coefficients(self) -> np.ndarray:
        n = C.c_uint32(0)
        p = self.lib.jda_coef_image_coefficients(self.handle, C.byref(n))
        return np.ctypeslib.as_array(C.cast(p, C.POINTER(C.c_int16)), shape=(n.value, 64)).copy() if n.value else np.zeros((0, 64), np.int16)

    def quant(self):
        """(4 x 64 prescaled quantisers in natural order, table ids of Y / Cb / Cr)"""
        ids = (C.c_uint8 * 3)()
        p = self.lib.jda_coef_image_quant(self.handle, ids)
        return np.ctypeslib.as_array(C.cast(p, C.POINTER(C.c_int16)), shape=(4, 64)).copy(), list(ids)

    def sparse(self):
        """(first, entries): the sparse form (jda_coef_image_sparse) as numpy views of the image's own arrays -- valid until close().
        first: uint32[blocks + 1]; entries: uint32, (block & 1023) << 22 | natural index << 16 | value & 0xffff, nonzero values only."""
        first, n = _P(), C.c_uint32(0)
        p = self.lib.jda_coef_image_sparse(self.handle, C.byref(first), C.byref(n))
        if not p:
            raise JdaError(self.lib.jda_coef_image_sparse_status(self.handle), "jda_coef_image_sparse")
        nb = C.c_uint32(0)
        self.lib.jda_coef_image_coefficients(self.handle, C.byref(nb))
        f = np.ctypeslib.as_array(C.cast(first, C.POINTER(C.c_uint32)), shape=(nb.value + 1,))
        e = np.ctypeslib.as_array(C.cast(p, C.POINTER(C.c_uint32)), shape=(n.value,)) if n.value else np.zeros(0, np.uint32)
        return f, e

    def sparse_bytes(self) -> int:
        return int(self.lib.jda_coef_image_sparse_bytes(self.handle))

    def dense_bytes(self) -> int:
        nb = C.c_uint32(0)
        self.lib.jda_coef_image_coefficients(self.handle, C.byref(nb))
        return (nb.value * 128 + 15) & ~15

    def geometry(self, pixel_type=RGB8888, options=0):
        return output_geometry(self.info, pixel_type, options | (PROGRESSIVE_FULL if self.info.jpeg_type == 1 else 0))

    def close(self):
        if self.handle:
            if self.owned:
                self.lib.jda_coef_image_free(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class DeviceCoef:
    """A coefficient image resident in HBM (jda_coef_upload_ex): form COEF_DENSE / COEF_SPARSE / COEF_AUTO."""

    def __init__(self, ctx: Context, image: CoefImage, form=COEF_DENSE):
        self.ctx = ctx
        err = C.c_int32(0)
        self.handle = ctx.lib.jda_coef_upload_ex(ctx.handle, image.handle, form, C.byref(err))
        if not self.handle:
            raise JdaError(err.value, "jda_coef_upload_ex")
        self.info = ImageInfo.from_buffer_copy(image.info)
        self.form = int(ctx.lib.jda_dev_coef_form(self.handle))

    def close(self):
        if self.handle:
            self.ctx.lib.jda_dev_coef_free(self.ctx.handle, self.handle)
            self.handle = None


def coef_decode(ctx: Context, images, pixel_types, options=None, form=COEF_DENSE, rects=None):
    """jda_coef_upload_ex + ONE jda_coef_decode_surfaces_rect over all the images: [(canvas, geometry)] in MCU-padded host canvases.
    form: COEF_DENSE / COEF_SPARSE / COEF_AUTO for all images, or one per image (dense and sparse images may share the call).
    rects: None, or per image None / (mx0, my0, mx1, my1) in MCUs (half open); the canvases start as zeros, which is what a rectangle leaves
    outside it.
    With the defaults (dense, no rectangles) the call is jda_coef_upload + jda_coef_decode_surfaces, as before."""
    n = len(images)
    options = list(options) if options is not None else [0] * n
    forms = [form] * n if isinstance(form, int) else list(form)
    geos = [im.geometry(pt, opt) for im, pt, opt in zip(images, pixel_types, options)]
    pitch = [(g["canvas_w"] * g["bpp"] + 15) & ~15 for g in geos]
    offs, total = [], 0
    for g, p in zip(geos, pitch):
        offs.append(total)
        total += (p * g["canvas_h"] + 255) & ~255
    devs, base = [], ctx.malloc(max(total, 256))
    plain = all(f == COEF_DENSE for f in forms) and rects is None
    try:
        if rects is not None:
            ctx.memset(base, 0, max(total, 256))
        for im, f in zip(images, forms):
            err = C.c_int32(0)
            d = ctx.lib.jda_coef_upload(ctx.handle, im.handle, C.byref(err)) if plain else ctx.lib.jda_coef_upload_ex(ctx.handle, im.handle, f, C.byref(err))
            if not d:
                raise JdaError(err.value, "jda_coef_upload")
            devs.append(d)
        outs = (Output * n)(*[Output(base + offs[i], pitch[i], geos[i]["canvas_w"], geos[i]["canvas_h"]) for i in range(n)])
        if plain:
            ctx.check(ctx.lib.jda_coef_decode_surfaces(ctx.handle, n, (_P * n)(*devs), outs, (C.c_int32 * n)(*pixel_types), (C.c_int32 * n)(*options)),
                      "jda_coef_decode_surfaces")
        else:
            r = None
            if rects is not None:
                flat = []
                for im, rc in zip(images, rects):
                    flat += list(rc) if rc is not None else [0, 0, im.info.mcus_x, im.info.mcus_y]
                r = (C.c_int32 * (4 * n))(*flat)
            ctx.check(ctx.lib.jda_coef_decode_surfaces_rect(ctx.handle, n, (_P * n)(*devs), outs, (C.c_int32 * n)(*pixel_types), (C.c_int32 * n)(*options), r),
                      "jda_coef_decode_surfaces_rect")
        res = []
        for i, g in enumerate(geos):
            res.append((ctx.to_host(base + offs[i], pitch[i] * g["canvas_h"]).reshape(g["canvas_h"], pitch[i])[:, : g["canvas_w"] * g["bpp"]].copy(), g))
        return res
    finally:
        for d in devs:
            ctx.lib.jda_dev_coef_free(ctx.handle, d)
        ctx.free(base)


def dither_geometry(canvas_w, canvas_h, pixel_type):
    """jda_dither_geometry: {"bits", "pitch", "bytes"} of the packed form of a GRAY8 canvas."""
    bits, pitch, nbytes = C.c_int32(0), C.c_int32(0), C.c_int64(0)
    rc = load_library().jda_dither_geometry(canvas_w, canvas_h, pixel_type, C.byref(bits), C.byref(pitch), C.byref(nbytes))
    if rc != 0:
        raise JdaError(rc, "jda_dither_geometry")
    return {"bits": bits.value, "pitch": pitch.value, "bytes": nbytes.value}


def dither_seed(jpeg: bytes, base=None) -> np.ndarray:
    """jda_dither_seed: what the error row holds before the first strip of this file (base: a main image's seed to write over)."""
    seed = np.zeros(DITHER_SEED_BYTES, np.uint8) if base is None else np.array(base, dtype=np.uint8, copy=True)
    rc = load_library().jda_dither_seed(jpeg, len(jpeg), 0 if base is None else 1, seed.ctypes.data_as(_P))
    if rc != 0:
        raise JdaError(rc, "jda_dither_seed")
    return seed


def dither_surfaces(ctx: Context, gray, strip_rows, pixel_types, packed, seeds=None):
    """jda_dither_surfaces: gray / packed = lists of (device_ptr, pitch_bytes, width_px, rows); one launch for all of them.
    seeds: None, or one uint8 array of DITHER_SEED_BYTES (or None) per canvas."""
    n = len(gray)
    g = (Output * n)(*[Output(*o) for o in gray])
    p = (Output * n)(*[Output(*o) for o in packed])
    keep = [None if (seeds is None or s is None) else np.ascontiguousarray(s, dtype=np.uint8) for s in (seeds or [None] * n)]
    sp = (_P * n)(*[None if s is None else s.ctypes.data for s in keep])
    ctx.check(ctx.lib.jda_dither_surfaces(ctx.handle, n, g, (C.c_int32 * n)(*strip_rows), (C.c_int32 * n)(*pixel_types), sp, p), "jda_dither_surfaces")


def decode_dither_to_host(ctx: Context, jpeg: bytes, pixel_type=ONE_BIT_DITHERED, options=0, seed=None):
    """jda_decode_dither_to_host: (rc, packed rows (canvas_h x pitch), geometry of the gray canvas + "bits", "pitch", "strip_rows")."""
    info = ImageInfo()
    rc = ctx.lib.jda_parse(jpeg, len(jpeg), C.byref(info))
    if rc != 0:
        raise JdaError(rc, "jda_parse")
    g = output_geometry(info, GRAY8, options)
    d = dither_geometry(g["canvas_w"], g["canvas_h"], pixel_type)
    g.update(bits=d["bits"], pitch=d["pitch"], strip_rows=g["canvas_h"] // info.mcus_y)
    packed = np.zeros((g["canvas_h"], d["pitch"]), dtype=np.uint8)
    sd = None if seed is None else np.ascontiguousarray(seed, dtype=np.uint8)
    nok = C.c_int32(0)
    rc = ctx.lib.jda_decode_dither_to_host(ctx.handle, jpeg, len(jpeg), pixel_type, options, None if sd is None else sd.ctypes.data_as(_P),
                                           packed.ctypes.data_as(_P), d["pitch"], g["canvas_h"], C.byref(nok))
    return rc, packed, g


def oriented_geometry(info: ImageInfo, pixel_type=RGB8888, options=0, orientation=None):
    """jda_oriented_geometry: {"bpp", "w", "h", "strip_rows"} of the image after its EXIF orientation (orientation None: the file's)."""
    vals = [C.c_int32(0) for _ in range(4)]
    rc = load_library().jda_oriented_geometry(C.byref(info), pixel_type, options, -1 if orientation is None else orientation, *[C.byref(v) for v in vals])
    if rc != 0:
        raise JdaError(rc, "jda_oriented_geometry")
    return dict(zip(("bpp", "w", "h", "strip_rows"), [v.value for v in vals]))


def orient_surfaces(ctx: Context, src, bytes_per_pixel, orientations, dst):
    """jda_orient_surfaces: src / dst = lists of (device_ptr, pitch_bytes, width_px, rows); one launch for all of them."""
    n = len(src)
    s = (Output * max(n, 1))(*[Output(*o) for o in src])
    d = (Output * max(n, 1))(*[Output(*o) for o in dst])
    ctx.check(ctx.lib.jda_orient_surfaces(ctx.handle, n, s, bytes_per_pixel, (C.c_int32 * max(n, 1))(*orientations), d), "jda_orient_surfaces")


def decode_oriented_to_host(ctx: Context, jpeg: bytes, pixel_type=RGB8888, options=0, orientation=None, out=None):
    """jda_decode_to_host_oriented: (rc, the oriented visible pixels (h x w * bpp bytes), geometry of the unrotated decode + "w", "h",
    "strip_rows", "orientation").  orientation None: the file's.  out: an array of that shape from an earlier call, to decode into."""
    info = ImageInfo()
    rc = ctx.lib.jda_parse(jpeg, len(jpeg), C.byref(info))
    if rc != 0:
        raise JdaError(rc, "jda_parse")
    g = output_geometry(info, pixel_type, options)
    t = oriented_geometry(info, pixel_type, options, orientation)
    g.update(w=t["w"], h=t["h"], strip_rows=t["strip_rows"], orientation=info.orientation if orientation is None else orientation)
    shape = (t["h"], t["w"] * t["bpp"])
    pixels = out if out is not None and out.shape == shape and out.dtype == np.uint8 and out.flags["C_CONTIGUOUS"] else np.zeros(shape, dtype=np.uint8)
    nok = C.c_int32(0)
    rc = ctx.lib.jda_decode_to_host_oriented(ctx.handle, jpeg, len(jpeg), pixel_type, options, -1 if orientation is None else orientation,
                                             pixels.ctypes.data_as(_P), t["w"] * t["bpp"], t["h"], C.byref(nok))
    g["mcus_decoded"] = nok.value
    return rc, pixels, g


def pack_surfaces(ctx: Context, src, src_bytes_per_pixel, dst, layout=PACK_HWC, elem_type=PACK_U8, table=None, rects=None):
    """jda_pack_surfaces: src = list of (device_ptr, pitch_bytes, width_px, rows) of RGB8888 (4) or GRAY8 (1) surfaces, dst = list of device
    pointers of the dense results, table = device pointer of the C x 256 lookup table (F16 / F32), rects = list of (x, y, w, h) or None: all
    of width_px x rows.  One launch for all of them."""
    n = len(src)
    s = (Output * max(n, 1))(*[Output(*o) for o in src])
    d = (_P * max(n, 1))(*dst)
    r = None if rects is None else (C.c_int32 * max(4 * n, 1))(*[v for q in rects for v in q])
    ctx.check(ctx.lib.jda_pack_surfaces(ctx.handle, n, s, src_bytes_per_pixel, r, layout, elem_type, table, d), "jda_pack_surfaces")


def decode_packed_to_host(ctx: Context, jpeg: bytes, options=0, layout=PACK_HWC, elem_type=PACK_U8, table=None):
    """jda_decode_to_host_packed: (rc, the dense visible pixels -- [h, w, C] or, with PACK_CHW, [C, h, w]; uint8, float16 or float32; None when
    the call refused --, {"w", "h", "channels", "mcus_decoded"}).  table: a numpy array of C x 256 elements of the result's type, or None."""
    info = ImageInfo()
    rc = ctx.lib.jda_parse(jpeg, len(jpeg), C.byref(info))
    if rc != 0:
        raise JdaError(rc, "jda_parse")
    channels = 1 if info.ncomp == 1 or (options & LUMA_ONLY) else 3
    dtype = PACK_DTYPES.get(elem_type, np.uint8)
    flat = np.zeros(info.width * info.height * channels, dtype=dtype)      # (at least the visible size at any scale)
    tab = None if table is None else np.ascontiguousarray(table)
    w, h, nok = C.c_int32(0), C.c_int32(0), C.c_int32(0)
    rc = ctx.lib.jda_decode_to_host_packed(ctx.handle, jpeg, len(jpeg), options, layout, elem_type, None if tab is None else tab.ctypes.data_as(_P),
                                           flat.ctypes.data_as(_P), flat.nbytes, C.byref(w), C.byref(h), C.byref(nok))
    g = {"w": w.value, "h": h.value, "channels": channels, "mcus_decoded": nok.value}
    if w.value == 0:
        return rc, None, g
    shape = (channels, h.value, w.value) if layout & PACK_CHW else (h.value, w.value, channels)
    return rc, flat[:w.value * h.value * channels].reshape(shape), g


def _scale_bias(scale_bias, channels):
    """None, or (scale, bias) / an array of 2 x channels values -> a ctypes float array: scale[0..C-1], bias[0..C-1]"""
    if scale_bias is None:
        return None
    v = np.ascontiguousarray(np.asarray(scale_bias, np.float32).reshape(-1))
    if v.size != 2 * channels:
        raise ValueError("scale_bias: %d scales and %d biases" % (channels, channels))
    return (C.c_float * v.size)(*[float(x) for x in v])


def unpack_surfaces(ctx: Context, src_ptrs, dst, bytes_per_pixel, layout=PACK_HWC, elem_type=PACK_U8, scale_bias=None):
    """jda_unpack_surfaces, the inverse of pack_surfaces: src_ptrs = device pointers of dense images (HWC / CHW, uint8 / float16 / float32),
    dst = list of (device_ptr, pitch_bytes, width_px, rows) of the RGB8888 (4: A = 0xFF) or GRAY8 (1) surfaces they become -- width_px x rows
    is the image's size.  scale_bias: None (255, 0), or (scale[C], bias[C]) for float elements (denormalise_params).  One launch."""
    n = len(src_ptrs)
    s = (_P * max(n, 1))(*src_ptrs)
    d = (Output * max(n, 1))(*[Output(*o) for o in dst])
    sb = _scale_bias(scale_bias, 3 if bytes_per_pixel == 4 else 1)
    ctx.check(ctx.lib.jda_unpack_surfaces(ctx.handle, n, s, layout, elem_type, sb, d, bytes_per_pixel), "jda_unpack_surfaces")


def encode_dense_to_host(ctx: Context, array, layout=PACK_HWC, sampling="4:2:0", quality=75, restart_interval=0, form="baseline", scale_bias=None, capacity=None):
    """jda_encode_dense_to_host: array = a numpy image [h, w, C] (PACK_HWC, | PACK_BGR) or [C, h, w] (PACK_CHW), or [h, w] gray; uint8, float16
    or float32; -> (rc, the file's bytes or None, the size the file has or needs).  form: "baseline", "optimize" or "progressive" (RECODE_*).
    A gray image takes the gray sampling whatever `sampling` says.  capacity: the host buffer's bytes (default: the bound)."""
    a = np.ascontiguousarray(array)
    if a.ndim == 2:
        a = a[None] if layout & PACK_CHW else a[..., None]
    if a.ndim != 3:
        raise ValueError("array: [h, w, C], [C, h, w] or [h, w]")
    channels, h, w = a.shape if layout & PACK_CHW else (a.shape[2], a.shape[0], a.shape[1])
    elem = {np.dtype(v): k for k, v in PACK_DTYPES.items()}.get(a.dtype)
    if elem is None:
        raise ValueError("array: uint8, float16 or float32")
    samp = ENCODE_GRAY if channels == 1 else _sampling(sampling)
    f = _recode_form(form)
    if capacity is not None:
        cap = capacity
    else:
        cap = encode_bound_progressive(w, h, samp) if f == RECODE_PROGRESSIVE else encode_bound(w, h, samp, restart_interval)
    buf = np.zeros(max(cap, 1), dtype=np.uint8)
    nbytes = C.c_int64(0)
    rc = ctx.lib.jda_encode_dense_to_host(ctx.handle, a.ctypes.data_as(_P), w, h, channels, layout, elem, _scale_bias(scale_bias, channels), samp, quality,
                                          restart_interval, f, buf.ctypes.data_as(_P), cap, C.byref(nbytes))
    return rc, (buf[:nbytes.value].tobytes() if rc == 0 and nbytes.value <= cap else None), nbytes.value


def resize_filter(resample) -> int:
    """a filter's name ("bilinear", "box", "hamming", "bicubic", "lanczos", any case) or id (RESIZE_*) -> its id; ValueError for anything else"""
    if isinstance(resample, str):
        if resample.lower() in RESIZE_FILTERS:
            return RESIZE_FILTERS[resample.lower()]
    elif isinstance(resample, int) and not isinstance(resample, bool) and resample in RESIZE_FILTERS.values():
        return resample
    raise ValueError("resample: one of %s, or RESIZE_BILINEAR .. RESIZE_LANCZOS; not %r" % (", ".join(repr(k) for k in RESIZE_FILTERS), resample))


def resize_surfaces(ctx: Context, src, bytes_per_pixel, dst, rects=None, filter=0):
    """jda_resize_surfaces[_ex]: src / dst = lists of (device_ptr, pitch_bytes, width_px, rows) of RGB8888 (4) or GRAY8 (1) surfaces -- a
    destination's width_px x rows is the output size --, rects = list of (x, y, w, h) or None: all of width_px x rows.  Pillow's
    resize(F, box), bit for bit, F = filter (RESIZE_BILINEAR by default, .. RESIZE_LANCZOS; one for the call); one launch for all of them."""
    n = len(src)
    s = (Output * max(n, 1))(*[Output(*o) for o in src])
    d = (Output * max(n, 1))(*[Output(*o) for o in dst])
    r = None if rects is None else (C.c_int32 * max(4 * n, 1))(*[v for q in rects for v in q])
    if filter == 0:
        ctx.check(ctx.lib.jda_resize_surfaces(ctx.handle, n, s, bytes_per_pixel, r, d), "jda_resize_surfaces")
    else:
        ctx.check(ctx.lib.jda_resize_surfaces_ex(ctx.handle, n, s, bytes_per_pixel, r, d, filter), "jda_resize_surfaces_ex")


def resize_surfaces_box(ctx: Context, src, bytes_per_pixel, dst, boxes, filter=0):
    """jda_resize_surfaces_box: resize_surfaces with Pillow's resize(size, F, box) for FLOAT boxes: boxes = list of (x0, y0, x1, y1), one a
    job, 0 <= x0 < x1 <= width_px and the same for y.  The ends are held as float32, as Pillow's C side holds them."""
    n = len(src)
    s = (Output * max(n, 1))(*[Output(*o) for o in src])
    d = (Output * max(n, 1))(*[Output(*o) for o in dst])
    b = None if boxes is None else (C.c_float * max(4 * n, 1))(*[float(v) for q in boxes for v in q])
    ctx.check(ctx.lib.jda_resize_surfaces_box(ctx.handle, n, s, bytes_per_pixel, b, d, filter), "jda_resize_surfaces_box")


REDUCE_MAX_FACTOR = 32


def reduce_geometry(box_w, box_h, fx, fy):
    """jda_reduce_geometry: (out_w, out_h) = (ceil(box_w / fx), ceil(box_h / fy)), Pillow's size of Image.reduce((fx, fy), box); JdaError
    for a size or a factor below 1 or a factor beyond REDUCE_MAX_FACTOR"""
    ow, oh = C.c_int32(0), C.c_int32(0)
    rc = load_library().jda_reduce_geometry(int(box_w), int(box_h), int(fx), int(fy), C.byref(ow), C.byref(oh))
    if rc != 0:
        raise JdaError(rc, "jda_reduce_geometry")
    return ow.value, oh.value


def reduce_surfaces(ctx: Context, src, bytes_per_pixel, factors, dst, boxes=None):
    """jda_reduce_surfaces: Pillow's Image.reduce((fx, fy), box), bit for bit, of every job in one launch.  src / dst = lists of (device_ptr,
    pitch_bytes, width_px, rows) of RGB8888 (4) or GRAY8 (1) surfaces -- a destination's width_px x rows must be reduce_geometry's --,
    factors = list of (fx, fy), boxes = list of (x0, y0, x1, y1) or None: every source whole."""
    n = len(src)
    s = (Output * max(n, 1))(*[Output(*o) for o in src])
    d = (Output * max(n, 1))(*[Output(*o) for o in dst])
    f = None if factors is None else (C.c_int32 * max(2 * n, 1))(*[int(v) for q in factors for v in q])
    b = None if boxes is None else (C.c_int32 * max(4 * n, 1))(*[int(v) for q in boxes for v in q])
    ctx.check(ctx.lib.jda_reduce_surfaces(ctx.handle, n, s, bytes_per_pixel, f, b, d), "jda_reduce_surfaces")


def thumbnail_plan(src_w, src_h, size, filter=RESIZE_BICUBIC, reducing_gap=2.0) -> dict:
    """jda_thumbnail_plan: what Image.thumbnail(size, F, reducing_gap) does to a src_w x src_h JPEG file -- out (w, h): the final size;
    scale: draft()'s; draft (w, h): the decoded size; factors (fx, fy) and reduce_box (x0, y0, x1, y1): the reduce step, (1, 1) without
    one; reduced (w, h): the image the resize reads; resize: whether there is one; box: its float box.  reducing_gap None (or 0): Pillow's
    None.  JdaError for what the call refuses (a plan it cannot run is never handed out)."""
    t = ThumbnailSteps()
    rc = load_library().jda_thumbnail_plan(int(src_w), int(src_h), int(size[0]), int(size[1]), int(filter), float(reducing_gap or 0.0), C.byref(t))
    if rc != 0:
        raise JdaError(rc, "jda_thumbnail_plan")
    return dict(out=(t.out_w, t.out_h), scale=t.scale, draft=(t.draft_w, t.draft_h), factors=(t.fx, t.fy), reduce_box=tuple(t.reduce_box),
                reduced=(t.reduced_w, t.reduced_h), resize=bool(t.resize), box=tuple(t.box))


def decode_to_host_thumbnail(ctx: Context, jpeg: bytes, size, filter=RESIZE_BICUBIC, reducing_gap=2.0, pixel_type=RGB8888):
    """jda_decode_to_host_thumbnail: np.asarray(im) after im = Image.open(file); im.thumbnail(size, F, reducing_gap) -- (rc, out_h x out_w x 4
    RGBA bytes (A = 0xFF) or out_h x out_w gray, (reduce launches, resize launches)); the pixels are None when the call refuses."""
    info = ImageInfo()
    rc = ctx.lib.jda_parse(jpeg, len(jpeg), C.byref(info))
    if rc != 0:
        raise JdaError(rc, "jda_parse")
    bpp = 1 if pixel_type == GRAY8 else 4
    t = ThumbnailSteps()
    rc = ctx.lib.jda_thumbnail_plan(info.width, info.height, int(size[0]), int(size[1]), int(filter), float(reducing_gap or 0.0), C.byref(t))
    launches = (C.c_int32 * 2)()
    if rc != 0:
        return rc, None, tuple(launches)
    canvas = np.zeros((t.out_h, t.out_w * bpp), dtype=np.uint8)
    ow, oh = C.c_int32(0), C.c_int32(0)
    rc = ctx.lib.jda_decode_to_host_thumbnail(ctx.handle, jpeg, len(jpeg), int(size[0]), int(size[1]), int(filter), float(reducing_gap or 0.0), pixel_type,
                                              canvas.ctypes.data_as(_P), canvas.shape[1], canvas.shape[0], C.byref(ow), C.byref(oh), launches)
    if rc != 0:
        return rc, None, tuple(launches)
    assert (ow.value, oh.value) == (t.out_w, t.out_h)
    return rc, (canvas.reshape(t.out_h, t.out_w, 4) if bpp == 4 else canvas), tuple(launches)


def _sampling(s):
    return ENCODE_SAMPLINGS[s] if isinstance(s, str) else int(s)


def encode_bound(w, h, sampling, restart_interval=0) -> int:
    """jda_encode_bound: a capacity no w x h file of that sampling ("gray", "4:4:4", "4:2:2", "4:2:0" or ENCODE_*) and interval passes"""
    b = C.c_int64()
    rc = load_library().jda_encode_bound(w, h, _sampling(sampling), restart_interval, C.byref(b))
    if rc != 0:
        raise JdaError(rc, "jda_encode_bound")
    return b.value


def encode_surfaces(ctx: Context, src, bytes_per_pixel, jobs, dst, capacities, flags=None):
    """jda_encode_surfaces[_ex]: src = list of (device_ptr, pitch_bytes, width_px, rows) of RGB8888 (4) or GRAY8 (1) surfaces; jobs = list of
    (x, y, w, h, sampling, quality, restart_interval); dst = device pointers, capacities = their bytes.  -> (file sizes, statuses): libjpeg's
    baseline file for every rectangle, written where it lies in HBM; ERROR_MEMORY and the size it needs for a file that does not fit.
    flags: None, or a word per job (ENCODE_OPTIMIZE: Pillow's optimize=True for that file) -- then the call is jda_encode_surfaces_ex."""
    n = len(src)
    s = (Output * max(n, 1))(*[Output(*o) for o in src])
    j = (EncodeJob * max(n, 1))(*[EncodeJob(q[0], q[1], q[2], q[3], _sampling(q[4]), q[5], q[6] if len(q) > 6 else 0, 0) for q in jobs])
    d = (C.c_void_p * max(n, 1))(*dst)
    c = (C.c_int64 * max(n, 1))(*capacities)
    nbytes, status = (C.c_int64 * max(n, 1))(), (C.c_int32 * max(n, 1))()
    if flags is None:
        ctx.check(ctx.lib.jda_encode_surfaces(ctx.handle, n, s, bytes_per_pixel, j, d, c, nbytes, status), "jda_encode_surfaces")
    else:
        if len(flags) != n:
            raise ValueError("flags: one word per job")
        f = (C.c_uint32 * max(n, 1))(*[int(v) for v in flags])
        ctx.check(ctx.lib.jda_encode_surfaces_ex(ctx.handle, n, s, bytes_per_pixel, j, f, d, c, nbytes, status), "jda_encode_surfaces_ex")
    return list(nbytes)[:n], list(status)[:n]


def encode_bound_progressive(w, h, sampling) -> int:
    """jda_encode_bound_progressive: a capacity no progressive w x h file of that sampling passes"""
    b = C.c_int64()
    rc = load_library().jda_encode_bound_progressive(w, h, _sampling(sampling), C.byref(b))
    if rc != 0:
        raise JdaError(rc, "jda_encode_bound_progressive")
    return b.value


def encode_surfaces_progressive(ctx: Context, src, bytes_per_pixel, jobs, dst, capacities):
    """jda_encode_surfaces_progressive: encode_surfaces' arguments (a job's restart interval must be 0) -> (file sizes, statuses): the
    progressive file libjpeg writes for every rectangle (Pillow's progressive=True), written where it lies in HBM."""
    n = len(src)
    s = (Output * max(n, 1))(*[Output(*o) for o in src])
    j = (EncodeJob * max(n, 1))(*[EncodeJob(q[0], q[1], q[2], q[3], _sampling(q[4]), q[5], q[6] if len(q) > 6 else 0, 0) for q in jobs])
    d = (C.c_void_p * max(n, 1))(*dst)
    c = (C.c_int64 * max(n, 1))(*capacities)
    nbytes, status = (C.c_int64 * max(n, 1))(), (C.c_int32 * max(n, 1))()
    ctx.check(ctx.lib.jda_encode_surfaces_progressive(ctx.handle, n, s, bytes_per_pixel, j, d, c, nbytes, status), "jda_encode_surfaces_progressive")
    return list(nbytes)[:n], list(status)[:n]


def transcode_to_host(ctx: Context, jpeg: bytes, size=None, sampling="4:2:0", quality=75, restart_interval=0, options=0, rect=None, capacity=None, optimize=False,
                      progressive=False):
    """jda_transcode_to_host[_ex]: decode (rect = (x, y, w, h) of the visible image, or all of it), resize to size = (out_w, out_h) where that
    differs, encode; -> (rc, the file's bytes or None, the size the file has or needs).  capacity: the host buffer's bytes (default: the bound).
    optimize: Huffman tables of the file's own (ENCODE_OPTIMIZE).  progressive: a progressive file (jda_transcode_to_host_progressive; its
    tables are always the file's own, so optimize changes nothing in it; restart_interval must be 0)."""
    if size is None:
        if rect is not None:
            size = (rect[2], rect[3])
        else:
            info = ImageInfo()
            rc = ctx.lib.jda_parse(jpeg, len(jpeg), C.byref(info))
            if rc != 0:
                raise JdaError(rc, "jda_parse")
            g = output_geometry(info, GRAY8 if info.ncomp == 1 else RGB8888, options)
            size = (g["out_w"], g["out_h"])
    if capacity is not None:
        cap = capacity
    else:
        cap = encode_bound_progressive(size[0], size[1], sampling) if progressive else encode_bound(size[0], size[1], sampling, restart_interval)
    buf = np.zeros(max(cap, 1), dtype=np.uint8)
    r = (C.c_int32 * 4)(*rect) if rect is not None else None
    nbytes = C.c_int64(0)
    if progressive:
        rc = ctx.lib.jda_transcode_to_host_progressive(ctx.handle, jpeg, len(jpeg), options, r, size[0], size[1], _sampling(sampling), quality, restart_interval,
                                                       buf.ctypes.data_as(_P), cap, C.byref(nbytes))
    elif optimize:
        rc = ctx.lib.jda_transcode_to_host_ex(ctx.handle, jpeg, len(jpeg), options, r, size[0], size[1], _sampling(sampling), quality, restart_interval,
                                              ENCODE_OPTIMIZE, buf.ctypes.data_as(_P), cap, C.byref(nbytes))
    else:
        rc = ctx.lib.jda_transcode_to_host(ctx.handle, jpeg, len(jpeg), options, r, size[0], size[1], _sampling(sampling), quality, restart_interval,
                                           buf.ctypes.data_as(_P), cap, C.byref(nbytes))
    return rc, (buf[:nbytes.value].tobytes() if rc in (0, 2) and nbytes.value <= cap else None), nbytes.value


def _recode_form(f):
    return RECODE_FORMS[f] if isinstance(f, str) else int(f)


def recode_xform(transform=None, crop=None, trim=False) -> RecodeXform:
    """a jda_recode_xform: transform None / "flip_h" / "flip_v" / "transpose" / "transverse" / "rot90" / "rot180" / "rot270" / "exif" or XF_*; crop
    (x, y, w, h) in source MCUs, applied before the operation (None: the whole image); trim: drop a partial MCU column or row of a mirrored
    axis (jpegtran -trim) where the job is refused without (jpegtran -perfect).  A RecodeXform or its six words pass through."""
    if isinstance(transform, RecodeXform):
        return transform
    x = RecodeXform()
    if isinstance(transform, (tuple, list)):
        x.op, x.flags = int(transform[0]), int(transform[1])
        crop = transform[2:6]
    else:
        x.op = RECODE_TRANSFORMS[transform] if transform is None or isinstance(transform, str) else int(transform)
        x.flags = XF_TRIM if trim else 0
    for k in range(4):
        x.mcu_rect[k] = int(crop[k]) if crop is not None else 0
    return x


def recode_geometry(info: ImageInfo, transform=None, crop=None, trim=False) -> ImageInfo:
    """jda_recode_geometry: the header of the file a recode with this transform writes (width, height and MCU grid of the turned region;
    orientation 0); JdaError with the job's refusal"""
    out = ImageInfo()
    rc = load_library().jda_recode_geometry(C.byref(info), C.byref(recode_xform(transform, crop, trim)), C.byref(out))
    if rc != 0:
        raise JdaError(rc, "jda_recode_geometry")
    return out


def recode_bound(info: ImageInfo, form="optimize", restart_interval=None, xform=None) -> int:
    """jda_recode_bound[_ex]: a capacity no recoded file of a source with this header passes (restart_interval None: the source's own);
    xform: what recode_xform takes -- the bound of the turned region's file"""
    b = C.c_int64()
    ri = -1 if restart_interval is None else restart_interval
    if xform is None:
        rc = load_library().jda_recode_bound(C.byref(info), _recode_form(form), ri, C.byref(b))
    else:
        rc = load_library().jda_recode_bound_ex(C.byref(info), C.byref(recode_xform(xform)), _recode_form(form), ri, C.byref(b))
    if rc != 0:
        raise JdaError(rc, "jda_recode_bound")
    return b.value


def recode_images(ctx: Context, sources, jobs, dst, capacities, xforms=None):
    """jda_recode_images: sources = DeviceImage (a resident baseline image) or DeviceCoef (a resident coefficient image) each; jobs = a
    (form, restart_interval) each -- form "baseline" / "optimize" / "progressive" or RECODE_*, restart_interval None (the source's own), 0 or
    1..65535; dst = device pointers, capacities = their bytes.  -> (file sizes, statuses): the source's own coefficients and quantisers under
    the entropy coding asked for, written where the file lies in HBM.  xforms: None, or what recode_xform takes a job (jda_recode_images_ex):
    the file of the job's region flipped, turned or transposed, still without a pixel in between."""
    n = len(sources)
    s = (RecodeSource * max(n, 1))(*[RecodeSource(q.handle, None) if isinstance(q, DeviceImage) else RecodeSource(None, q.handle) for q in sources])
    j = (RecodeJob * max(n, 1))(*[RecodeJob(_recode_form(q[0]), -1 if q[1] is None else q[1], 0, 0) for q in jobs])
    d = (C.c_void_p * max(n, 1))(*dst)
    c = (C.c_int64 * max(n, 1))(*capacities)
    nbytes, status = (C.c_int64 * max(n, 1))(), (C.c_int32 * max(n, 1))()
    if xforms is None:
        ctx.check(ctx.lib.jda_recode_images(ctx.handle, n, s, j, d, c, nbytes, status), "jda_recode_images")
    else:
        x = xforms if isinstance(xforms, C.Array) else (RecodeXform * max(n, 1))(*[recode_xform(q) for q in xforms])      # (an array made before: no marshalling a call)
        ctx.check(ctx.lib.jda_recode_images_ex(ctx.handle, n, s, j, x, d, c, nbytes, status), "jda_recode_images_ex")
    return list(nbytes)[:n], list(status)[:n]


def recode_to_host(ctx: Context, jpeg: bytes, form="optimize", restart_interval=None, capacity=None, transform=None, crop=None, trim=False):
    """jda_recode_to_host[_ex]: a baseline or progressive file in, the same coefficients under another entropy coding out; -> (rc, the file's bytes
    or None, the size the file has or needs).  capacity: the host buffer's bytes (default: the bound).  transform, crop, trim: recode_xform's."""
    xf = None if transform is None and crop is None and not trim else recode_xform(transform, crop, trim)
    if capacity is not None:
        cap = capacity
    else:
        info = ImageInfo()
        rc = ctx.lib.jda_parse(jpeg, len(jpeg), C.byref(info))
        if rc != 0:
            raise JdaError(rc, "jda_parse")
        try:
            cap = recode_bound(info, form, restart_interval, xf)
        except JdaError as e:              # (a form, an interval or a layout the call refuses: its code, as the call itself gives it)
            return e.code, None, 0
    buf = np.zeros(max(cap, 1), dtype=np.uint8)
    nbytes = C.c_int64(0)
    if xf is None:
        rc = ctx.lib.jda_recode_to_host(ctx.handle, jpeg, len(jpeg), _recode_form(form), -1 if restart_interval is None else restart_interval, buf.ctypes.data_as(_P), cap,
                                        C.byref(nbytes))
    else:
        rc = ctx.lib.jda_recode_to_host_ex(ctx.handle, jpeg, len(jpeg), _recode_form(form), -1 if restart_interval is None else restart_interval, C.byref(xf),
                                           buf.ctypes.data_as(_P), cap, C.byref(nbytes))
    return rc, (buf[:nbytes.value].tobytes() if rc == 0 and nbytes.value <= cap else None), nbytes.value


def recode(ctx: Context, files, form="optimize", transform=None, crop=None, trim=False):
    """Baseline files in, a list of bytes out: prepare_batch with the device pre-scan, upload_batch and ONE recode_images call (a file the
    call refuses raises JdaError with its status).  transform, crop, trim: recode_xform's, the same for every file -- transform="exif" turns
    each file by its own orientation tag, so a mixed list comes out upright."""
    xf = None if transform is None and crop is None and not trim else recode_xform(transform, crop, trim)
    prepared = prepare_batch(list(files), device_prescan=True)
    images = []
    base = None
    try:
        images = upload_batch(ctx, prepared)
        caps = [recode_bound(im.info, form, None, xf) for im in images]
        offs, total = [], 0
        for c in caps:
            offs.append(total)
            total += (c + 255) & ~255
        base = ctx.malloc(max(total, 256))
        nbytes, status = recode_images(ctx, images, [(form, None)] * len(images), [base + o for o in offs], caps, None if xf is None else [xf] * len(images))
        for st in status:
            if st != 0:
                raise JdaError(st, "jda_recode_images")
        return [ctx.to_host(base + o, nb).tobytes() for o, nb in zip(offs, nbytes)]
    finally:
        if base is not None:
            ctx.free(base)
        for im in images:
            if im is not None:
                im.close()
        for p in prepared:
            if p is not None:
                p.close()


def _recode_sources(sources):
    n = len(sources)
    return (RecodeSource * max(n, 1))(*[RecodeSource(q.handle, None) if isinstance(q, DeviceImage) else RecodeSource(None, q.handle) for q in sources])


# the colour models of jda_exact_probe (jdapimin.c's rule) and the flag of the _ex calls that makes them decide
CMYK8888 = 16                                     # JDA_CMYK8888: Pillow's mode-"CMYK" bytes of a four-component source (the exact decode with colour_models=True)
CS_GRAY, CS_YCBCR, CS_RGB, CS_CMYK, CS_YCCK = 0, 1, 2, 3, 4
CS_NAMES = {CS_GRAY: "gray", CS_YCBCR: "ycbcr", CS_RGB: "rgb", CS_CMYK: "cmyk", CS_YCCK: "ycck"}
EXACT_COLOUR_MODELS = 1


class ExactFile(C.Structure):
    _fields_ = [("colour_model", C.c_int32), ("ncomp", C.c_int32), ("layout", C.c_int32), ("k_sampling", C.c_int32), ("width", C.c_int32), ("height", C.c_int32),
                ("jpeg_type", C.c_int32), ("decodable", C.c_int32), ("jfif", C.c_int32), ("adobe", C.c_int32), ("adobe_transform", C.c_int32),
                ("component_id", C.c_int32 * 4)]


def exact_probe(jpeg: bytes):
    """jda_exact_probe: how libjpeg reads the file's components -- {"colour_model": CS_*, "model": its name, "ncomp", "layout" (0 gray, 1 4:4:4,
    2 4:2:0, 3 4:2:2, 4 4:4:0, -1 another), "k_sampling", "width", "height", "progressive", "decodable" (by the exact calls with
    colour_models=True), "jfif", "adobe", "adobe_transform", "component_ids"}; a header jda_parse refuses raises JdaError."""
    f = ExactFile()
    rc = load_library().jda_exact_probe(jpeg, len(jpeg), C.byref(f))
    if rc != 0 and (rc != 3 or f.colour_model < 0):          # (JDA_UNSUPPORTED_FEATURE behind a header that parsed: the fields stand, decodable is False)
        raise JdaError(rc, "jda_exact_probe")
    return dict(colour_model=f.colour_model, model=CS_NAMES.get(f.colour_model), ncomp=f.ncomp, layout=f.layout, k_sampling=f.k_sampling, width=f.width,
                height=f.height, progressive=bool(f.jpeg_type), decodable=bool(f.decodable), jfif=bool(f.jfif), adobe=bool(f.adobe),
                adobe_transform=f.adobe_transform, component_ids=list(f.component_id)[:f.ncomp])


def exact_decode(ctx: Context, sources, outputs, pixel_types=None, scales=None, colour_models=False, rects=None):
    """jda_exact_decode_surfaces: the libjpeg-exact decode (Pillow's pixels, not the reference's) of resident sources -- DeviceImage (a
    baseline file) or DeviceCoef (dense or sparse) each -- into surfaces.  outputs = (device pointer, pitch, width_px, rows) each;
    pixel_types: RGB8888 (the default) or GRAY8 each.  Exactly min(width, width_px) x min(height, rows) pixels of an image are written.
    scales (jda_exact_decode_surfaces_scaled): 1, 2, 4 or 8 each -- libjpeg's scaled decode, Pillow's draft(); the image is then
    ceil(width / s) x ceil(height / s).  colour_models (jda_exact_decode_surfaces_ex with JDA_EXACT_COLOUR_MODELS): a file with an Adobe
    segment is taken, an RGB-coded one (exact_probe) is written as R, G, B, and a four-component DeviceCoef of CoefImage.from_file (CMYK,
    YCCK; scale 1) as Pillow's convert("RGB") of it, or, pixel type CMYK8888, as Pillow's mode-"CMYK" bytes.
    rects (jda_exact_decode_surfaces_rect): (x, y, w, h) each, in pixels of the image at its scale, or None / (0, 0, 0, 0) for that image
    whole -- only the MCUs the rectangle's pixels read are decoded (exact_rect_mcus) and the surface holds the rectangle: exactly
    min(w, width_px) x min(h, rows) pixels are written.  -> the statuses; the call's own refusals raise JdaError."""
    n = len(sources)
    o = (Output * max(n, 1))(*[Output(*q) for q in outputs])
    pt = None if pixel_types is None else (C.c_int32 * max(n, 1))(*pixel_types)
    status = (C.c_int32 * max(n, 1))()
    if rects is not None:
        flat = [int(v) for r in rects for v in (r if r is not None else (0, 0, 0, 0))]
        sc = None if scales is None else (C.c_int32 * max(n, 1))(*scales)
        ctx.check(ctx.lib.jda_exact_decode_surfaces_rect(ctx.handle, n, _recode_sources(sources), o, pt, sc, EXACT_COLOUR_MODELS if colour_models else 0,
                                                         (C.c_int32 * max(4 * n, 1))(*flat), status), "jda_exact_decode_surfaces_rect")
        return list(status)[:n]
    if colour_models:
        sc = None if scales is None else (C.c_int32 * max(n, 1))(*scales)
        ctx.check(ctx.lib.jda_exact_decode_surfaces_ex(ctx.handle, n, _recode_sources(sources), o, pt, sc, EXACT_COLOUR_MODELS, status), "jda_exact_decode_surfaces_ex")
    elif scales is None:
        ctx.check(ctx.lib.jda_exact_decode_surfaces(ctx.handle, n, _recode_sources(sources), o, pt, status), "jda_exact_decode_surfaces")
    else:
        sc = (C.c_int32 * max(n, 1))(*scales)
        ctx.check(ctx.lib.jda_exact_decode_surfaces_scaled(ctx.handle, n, _recode_sources(sources), o, pt, sc, status), "jda_exact_decode_surfaces_scaled")
    return list(status)[:n]


def exact_planes(ctx: Context, sources, planes, scales=None, colour_models=False):
    """jda_exact_decode_planes: the 8-bit component planes at their own extents (libjpeg's raw-data output).  planes = per source three
    (device pointer, pitch, width, rows) -- Y, Cb, Cr; a gray image's last two are not looked at.  scales (jda_exact_decode_planes_scaled):
    1, 2, 4 or 8 each, the extents then exact_scaled_geometry's.  colour_models (jda_exact_decode_planes_ex): as exact_decode's -- an RGB-coded
    file's planes are R, G, B, and a four-component source takes FOUR entries (the fourth: K at its own extent, un-inverted; the call's
    array holds four an image, a shorter list here is padded).  -> the statuses."""
    n = len(sources)
    status = (C.c_int32 * max(n, 1))()
    if colour_models:                                        # (four entries a source: a three-tuple is padded with an entry nobody looks at)
        flat = [Output(*q) for some in planes for q in (list(some) + [(None, 0, 0, 0)])[:4]]
        sc = None if scales is None else (C.c_int32 * max(n, 1))(*scales)
        ctx.check(ctx.lib.jda_exact_decode_planes_ex(ctx.handle, n, _recode_sources(sources), (Output * max(4 * n, 1))(*flat), sc, EXACT_COLOUR_MODELS, status),
                  "jda_exact_decode_planes_ex")
        return list(status)[:n]
    flat = [Output(*q) for three in planes for q in three]
    if scales is None:
        ctx.check(ctx.lib.jda_exact_decode_planes(ctx.handle, n, _recode_sources(sources), (Output * max(3 * n, 1))(*flat), status), "jda_exact_decode_planes")
    else:
        sc = (C.c_int32 * max(n, 1))(*scales)
        ctx.check(ctx.lib.jda_exact_decode_planes_scaled(ctx.handle, n, _recode_sources(sources), (Output * max(3 * n, 1))(*flat), sc, status), "jda_exact_decode_planes_scaled")
    return list(status)[:n]


def _info_of(jpeg_or_info):
    if isinstance(jpeg_or_info, ImageInfo):
        return jpeg_or_info
    info = ImageInfo()
    rc = load_library().jda_parse(jpeg_or_info, len(jpeg_or_info), C.byref(info))
    if rc != 0:
        raise JdaError(rc, "jda_parse")
    return info


def exact_scaled_geometry(jpeg_or_info, scale):
    """jda_exact_scaled_geometry of a file (bytes) or an ImageInfo: {"width", "height": the output at that scale, "components": [(w, h)] the own
    extents of Y, Cb, Cr}; a scale outside 1, 2, 4, 8 raises JdaError."""
    info = _info_of(jpeg_or_info)
    w, h, cw, ch = C.c_int32(), C.c_int32(), (C.c_int32 * 3)(), (C.c_int32 * 3)()
    rc = load_library().jda_exact_scaled_geometry(C.byref(info), scale, C.byref(w), C.byref(h), cw, ch)
    if rc != 0:
        raise JdaError(rc, "jda_exact_scaled_geometry")
    return dict(width=w.value, height=h.value, components=[(cw[c], ch[c]) for c in range(info.ncomp)])


def exact_draft_scale(jpeg_or_info, size):
    """jda_exact_draft_scale: the scale Pillow's Image.draft(mode, size) chooses for the file; size = (width, height) as Pillow's"""
    info = _info_of(jpeg_or_info)
    return load_library().jda_exact_draft_scale(C.byref(info), int(size[0]), int(size[1]))


def exact_rect_mcus(jpeg_or_info, rect, scale=1, pixel_type=RGB8888):
    """jda_exact_rect_mcus: the half-open MCU rectangle (mx0, my0, mx1, my1) exact_decode(.., rects=) decodes for rect = (x, y, w, h), pixels of
    the image at `scale` (a gray surface of a colour file decodes no chroma); a rectangle the decode refuses raises JdaError."""
    info = _info_of(jpeg_or_info)
    out = (C.c_int32 * 4)()
    rc = load_library().jda_exact_rect_mcus(C.byref(info), scale, pixel_type, (C.c_int32 * 4)(*[int(v) for v in rect]), out)
    if rc != 0:
        raise JdaError(rc, "jda_exact_rect_mcus")
    return tuple(out)


def resize_reads(src_size, rect, out_size, filter=0):
    """jda_resize_reads: the source rectangle (x0, y0, x1, y1), half open, that resizing rect = (x, y, w, h) of a src_size = (w, h) image to
    out_size = (w, h) reads with `filter` (RESIZE_*), clipped at the image"""
    out = (C.c_int32 * 4)()
    rc = load_library().jda_resize_reads(int(src_size[0]), int(src_size[1]), (C.c_int32 * 4)(*[int(v) for v in rect]), int(out_size[0]), int(out_size[1]), filter, out)
    if rc != 0:
        raise JdaError(rc, "jda_resize_reads")
    return tuple(out)


def decode_to_host_exact(ctx: Context, jpeg: bytes, pixel_type=RGB8888, scale=1, colour_models=False, rect=None):
    """jda_decode_to_host_exact[_scaled]: one file, baseline or progressive, to the pixels Pillow gives (at scale 2, 4, 8: after
    draft()) -- (rc, height x width x 4 RGBA bytes or height x width gray).  colour_models (jda_decode_to_host_exact_ex): as exact_decode's.
    rect = (x, y, w, h) (jda_decode_to_host_exact_rect): that rectangle of the image at its scale alone -- (rc, h x w [x 4] pixels,
    (planes-stage tiles launched, those of the whole image))."""
    bpp = 4 if pixel_type in (RGB8888, CMYK8888) else 1
    if rect is not None:
        x, y, w, h = [int(v) for v in rect]
        canvas = np.zeros((max(h, 1), max(w, 1) * bpp), dtype=np.uint8)
        tiles = (C.c_int32 * 2)()
        rc = ctx.lib.jda_decode_to_host_exact_rect(ctx.handle, jpeg, len(jpeg), pixel_type, scale, EXACT_COLOUR_MODELS if colour_models else 0, (C.c_int32 * 4)(x, y, w, h),
                                                   canvas.ctypes.data_as(_P), canvas.shape[1], canvas.shape[0], tiles)
        return rc, (canvas.reshape(canvas.shape[0], -1, 4) if bpp == 4 else canvas), tuple(tiles)
    if colour_models:
        p = exact_probe(jpeg)                                     # (jda_parse refuses an extended-sequential frame, which this road takes)
        s = scale if scale in (1, 2, 4, 8) else 1
        w, h = -(-p["width"] // s), -(-p["height"] // s)
        canvas = np.zeros((h, w * bpp), dtype=np.uint8)
        rc = ctx.lib.jda_decode_to_host_exact_ex(ctx.handle, jpeg, len(jpeg), pixel_type, scale, EXACT_COLOUR_MODELS, canvas.ctypes.data_as(_P), canvas.shape[1],
                                                 canvas.shape[0])
        return rc, (canvas.reshape(h, w, 4) if bpp == 4 else canvas)
    info = ImageInfo()
    rc = ctx.lib.jda_parse(jpeg, len(jpeg), C.byref(info))
    if rc != 0:
        raise JdaError(rc, "jda_parse")
    if scale == 1:
        canvas = np.zeros((info.height, info.width * bpp), dtype=np.uint8)
        rc = ctx.lib.jda_decode_to_host_exact(ctx.handle, jpeg, len(jpeg), pixel_type, canvas.ctypes.data_as(_P), canvas.shape[1], canvas.shape[0])
        return rc, (canvas.reshape(info.height, info.width, 4) if bpp == 4 else canvas)
    s = scale if scale in (2, 4, 8) else 1                          # (a scale the call refuses: a canvas of the file's size, left untouched)
    w, h = -(-info.width // s), -(-info.height // s)
    canvas = np.zeros((h, w * bpp), dtype=np.uint8)
    rc = ctx.lib.jda_decode_to_host_exact_scaled(ctx.handle, jpeg, len(jpeg), pixel_type, scale, canvas.ctypes.data_as(_P), canvas.shape[1], canvas.shape[0])
    return rc, (canvas.reshape(h, w, 4) if bpp == 4 else canvas)


def decode_resized_to_host(ctx: Context, jpeg: bytes, size, pixel_type=RGB8888, options=0, rect=None, out=None, filter=0):
    """jda_decode_to_host_resized[_ex] (filter: RESIZE_*, the triangle by default): size = (out_w, out_h), rect = (x, y, w, h) in pixels of the visible image at the options' scale, or None:
    all of it.  (rc, the resized pixels [out_h, out_w * bpp] uint8, geometry of the decode + "mcus_decoded", (tiles launched, tiles of the
    whole image)).  out: the caller's 2-D uint8 array to decode into, its row stride is the pitch handed to the call."""
    info = ImageInfo()
    rc = ctx.lib.jda_parse(jpeg, len(jpeg), C.byref(info))
    if rc != 0:
        raise JdaError(rc, "jda_parse")
    out_w, out_h = size
    bpp = 1 if pixel_type == GRAY8 else 4
    pixels = out if out is not None else np.zeros((max(out_h, 1), max(out_w, 1) * bpp), dtype=np.uint8)
    if pixels.dtype != np.uint8 or pixels.ndim != 2 or not pixels.flags["WRITEABLE"] or pixels.strides[1] != 1:
        raise ValueError("out: a writable 2-D uint8 array, its last axis contiguous")
    r = (C.c_int32 * 4)(*rect) if rect is not None else None
    tiles = (C.c_int32 * 2)()
    nok = C.c_int32(0)
    if filter == 0:
        rc = ctx.lib.jda_decode_to_host_resized(ctx.handle, jpeg, len(jpeg), pixel_type, options, r, out_w, out_h, pixels.ctypes.data_as(_P), pixels.strides[0],
                                                pixels.shape[0], C.byref(nok), tiles)
    else:
        rc = ctx.lib.jda_decode_to_host_resized_ex(ctx.handle, jpeg, len(jpeg), pixel_type, options, r, out_w, out_h, filter, pixels.ctypes.data_as(_P),
                                                   pixels.strides[0], pixels.shape[0], C.byref(nok), tiles)
    try:
        g = output_geometry(info, pixel_type, options)
    except JdaError:
        g = {}
    g["mcus_decoded"] = nok.value
    return rc, pixels, g, (tiles[0], tiles[1])


def decode_resident(ctx: Context, prepared: PreparedImage, pixel_type=RGB8888, options=0):
    """One prepared image through jda_upload + jda_batch_create + jda_batch_decode into an MCU-padded host canvas:
    (status of the image, canvas, geometry) -- the path on which an image keeps what its jda_prepare_ex flags asked for."""
    g = prepared.geometry(pixel_type, options)
    pitch = (g["canvas_w"] * g["bpp"] + 15) & ~15
    dimg = DeviceImage(ctx, prepared)
    surf = ctx.malloc(pitch * g["canvas_h"])
    try:
        ctx.memset(surf, 0, pitch * g["canvas_h"])
        batch = Batch(ctx, [dimg], [(surf, pitch, g["canvas_w"], g["canvas_h"])], [pixel_type], [options])
        try:
            batch.decode()
            ctx.sync()
            st = batch.status()[0]
        finally:
            batch.close()
        canvas = ctx.to_host(surf, pitch * g["canvas_h"]).reshape(g["canvas_h"], pitch)[:, : g["canvas_w"] * g["bpp"]].copy()
    finally:
        ctx.free(surf)
        dimg.close()
    return st, canvas, g


def kernel_launch_counts() -> dict:
    """jda_kernel_launch_counts: {kernel symbol: launches} for every kernel this process has launched so far."""
    lib = load_library()
    need = lib.jda_kernel_launch_counts(None, 0)
    buf = C.create_string_buffer(need + 4096)
    lib.jda_kernel_launch_counts(buf, len(buf))
    out = {}
    for line in buf.value.decode().splitlines():
        name, _, n = line.rpartition(" ")
        out[name] = int(n)
    return out


def decode_to_host_rect(ctx: Context, jpeg: bytes, pixel_type, options, mcu_rect, out=None):
    """jda_decode_to_host_rect: (rc, canvas, geometry, (tiles launched, tiles of the whole image)); the geometry carries "mcus_decoded".
    out: the caller's 2-D uint8 array to decode into -- at least canvas_h rows, its row stride is the pitch handed to the call (at least
    a canvas row's bytes), its last axis contiguous; it is returned as the canvas."""
    info = ImageInfo()
    rc = ctx.lib.jda_parse(jpeg, len(jpeg), C.byref(info))
    if rc != 0:
        raise JdaError(rc, "jda_parse")
    g = output_geometry(info, pixel_type, options)
    if out is None:
        canvas = np.zeros((g["canvas_h"], g["canvas_w"] * g["bpp"]), dtype=np.uint8)
    else:
        canvas = out
        if (canvas.dtype != np.uint8 or canvas.ndim != 2 or not canvas.flags["WRITEABLE"] or canvas.strides[1] != 1 or canvas.shape[0] < g["canvas_h"]
                or canvas.shape[1] < g["canvas_w"] * g["bpp"] or canvas.strides[0] < canvas.shape[1]):
            raise ValueError("out: a writable 2-D uint8 array of at least canvas_h rows x canvas_w * bpp bytes")
    rect = (C.c_int32 * 4)(*mcu_rect) if mcu_rect is not None else None
    tiles = (C.c_int32 * 2)()
    nok = C.c_int32(0)
    rc = ctx.lib.jda_decode_to_host_rect(ctx.handle, jpeg, len(jpeg), pixel_type, options, rect, canvas.ctypes.data_as(_P), canvas.strides[0],
                                         canvas.shape[0], C.byref(nok), tiles)
    g["mcus_decoded"] = nok.value
    return rc, canvas, g, (tiles[0], tiles[1])


def filter_on_device(ctx: Context, raw: bytes, restart_cap: int = 1 << 16):
    """JPEGFilter on the GPU (jda_filter_on_device): (filtered bytes, restart positions incl. the leading 0)."""
    out = np.zeros(max(len(raw), 1), np.uint8)
    n, nr = C.c_int32(0), C.c_int32(0)
    rpos = np.zeros(restart_cap, np.uint32)
    rc = ctx.lib.jda_filter_on_device(ctx.handle, raw, len(raw), out.ctypes.data_as(_P), C.byref(n), rpos.ctypes.data_as(_P), restart_cap, C.byref(nr))
    if rc != 0:
        raise JdaError(rc, "jda_filter_on_device")
    return out[: n.value].tobytes(), rpos[: min(nr.value + 1, restart_cap)].copy(), nr.value
