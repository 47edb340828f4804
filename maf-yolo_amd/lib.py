"""ctypes binding of libmafyolo_hip.so (C-ABI: include/mafyolo_hip.h).

The product path has no CPU fallback: if the library is missing this raises, loudly."""
import ctypes as C
import os

from .config import cfg

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = cfg.hip_lib or os.path.join(_HERE, "libmafyolo_hip.so")     # MAF_HIP_LIB: an instrumented build (make prof)

F16, F32, U8 = 0, 1, 2
NMS_FLOAT_THRESHOLD = 1
NMS_PRECOLLECTED = 4         # maf_nms_ex flag: the forward pass (maf_engine_run_filtered) has written the candidate lists of the workspace
NMS_CNT_STRIDE = 64           # MAF_NMS_CNT_STRIDE: ints between the counter lines of two images at the start of the NMS workspace
NMS_MATRIX = 8                # maf_nms_ex flag: the all-pairs path as suppression matrix + scan (rounds 2-5) instead of the kept-list scan (A/B)
NMS_SINGLE_LAUNCH = 2         # maf_nms_ex flag: one launch (collect, then the last workgroup of every image sorts and selects) — the latency path
ACT_NONE, ACT_RELU, ACT_SILU, ACT_SIGMOID = 0, 1, 2, 3
SRC_DIRECT, SRC_UP2, SRC_POOL2, SRC_SUB2, SRC_PAIRS = 0, 1, 2, 3, 4
OP_STEM, OP_CONV1X1, OP_CONV3X3S2, OP_DWCONV, OP_SPPF_POOL, OP_DECODE, OP_BOTTLENECK, OP_CONV1DW, OP_HEADTAIL, OP_STEM2, OP_CONV3X3S2_DGRAD = range(11)
# MAF_CONV_* / MAF_CONV3_*: the kernel variant a conv op's tile_k selects (0 = CONV_GENERIC in the forward dispatch)
CONV_GENERIC, CONV_LDS, CONV_STREAM, CONV_SPLITK, CONV_STREAM_LDS, CONV3_LDS, CONV3_WREG, CONV_DMA = range(1, 9)
CONV_VARIANT_NAMES = {CONV_GENERIC: "generic", CONV_LDS: "lds", CONV_STREAM: "stream", CONV_SPLITK: "k4", CONV_STREAM_LDS: "streamlds", CONV3_LDS: "ldsall",
                      CONV3_WREG: "wreg", CONV_DMA: "dma"}
DW_MFMA, DW_DOT2, DW_PAIRS = -1, -2, -4       # MAF_DW_*: the kernel a depth-wise op's negative tile_p selects
DW_P2_STAGED = 128                            # MAF_DW_P2_STAGED: staged stores of the DW_PAIRS kernel, a bit of its tile_k


def dw_tile_k(rows, low, staged=False):
    """tile_k of a DW_DOT2 (low = channels per block) or DW_PAIRS (low = waves per workgroup) launch with `rows` tile rows."""
    return rows * 256 + low + (DW_P2_STAGED if staged else 0)


def dw_tile_k_split(tile_k):
    """(rows, low, staged) of such a tile_k."""
    return tile_k >> 8, tile_k & (DW_P2_STAGED - 1), bool(tile_k & DW_P2_STAGED)


class MafSrc(C.Structure):
    _fields_ = [("ptr", C.c_void_p), ("C", C.c_int32), ("stride", C.c_int32), ("coff", C.c_int32), ("mode", C.c_int32)]


class MafPackDesc(C.Structure):
    """maf_pack_desc_t (include/mafyolo_hip.h): one weight transform of maf_pack_batch."""
    _fields_ = [("src", C.c_void_p), ("dst", C.c_void_p), ("total", C.c_int64), ("kind", C.c_int32), ("dtype", C.c_int32),
                ("Cout", C.c_int32), ("Cin", C.c_int32), ("taps", C.c_int32), ("transpose", C.c_int32),
                ("CT", C.c_int32), ("steps", C.c_int32), ("Kp", C.c_int32), ("flip", C.c_int32), ("block0", C.c_int32), ("reserved", C.c_int32)]


class MafLetterboxImage(C.Structure):
    """maf_letterbox_image_t (include/mafyolo_hip.h): one frame of maf_letterbox."""
    _fields_ = [("ptr", C.c_void_p), ("pitch", C.c_int64), ("h", C.c_int32), ("w", C.c_int32),
                ("new_h", C.c_int32), ("new_w", C.c_int32), ("top", C.c_int32), ("left", C.c_int32)]


LETTERBOX_KARG_MAX = 64       # MAF_LETTERBOX_KARG_MAX: frames whose table travels as kernel arguments; larger batches pass a device copy


class MafAugmentFrame(C.Structure):
    """maf_augment_frame_t (include/mafyolo_hip.h): one resize of maf_augment_resize."""
    _fields_ = [("src", C.c_void_p), ("src_pitch", C.c_int64), ("h", C.c_int32), ("w", C.c_int32),
                ("dst", C.c_void_p), ("new_h", C.c_int32), ("new_w", C.c_int32)]


AREA_FAST2, AREA_FASTN, AREA_GENERAL = 0, 1, 2      # MAF_AREA_*: the path of a maf_resize_area frame
AUGMENT_MAX_TILES = 4         # MAF_AUGMENT_MAX_TILES


class MafAugmentTile(C.Structure):
    """maf_augment_tile_t: a frame placed on the virtual canvas of maf_mosaic_affine."""
    _fields_ = [("ptr", C.c_void_p), ("pitch", C.c_int64), ("h", C.c_int32), ("w", C.c_int32),
                ("x0", C.c_int32), ("y0", C.c_int32), ("x1", C.c_int32), ("y1", C.c_int32), ("dx", C.c_int32), ("dy", C.c_int32)]


class MafAugmentSample(C.Structure):
    """maf_augment_sample_t: one sample of maf_mosaic_affine (inverse affine per layer, tiles, mixup ratio, flags, HSV tables)."""
    _fields_ = [("minv", (C.c_double * 6) * 2), ("r", C.c_double), ("ntiles", C.c_int32 * 2), ("hsv", C.c_int32), ("flipud", C.c_int32),
                ("fliplr", C.c_int32), ("reserved", C.c_int32), ("tile", (MafAugmentTile * AUGMENT_MAX_TILES) * 2), ("lut", (C.c_uint8 * 256) * 3)]


class MafAugmentPaste(C.Structure):
    """maf_augment_paste_t: the copy_paste masks of one sample of maf_mosaic_affine_paste (NULL: nothing pasted in that layer) and the canvas side."""
    _fields_ = [("mask", C.c_void_p * 2), ("C", C.c_int32), ("reserved", C.c_int32)]


POLYGON_COORD_MAX = 32767     # MAF_POLYGON_COORD_MAX: |vertex coordinate| maf_polygon_mask accepts
PR_MAX_DET = 1024             # MAF_PR_MAX_DET / MAF_PR_MAX_LABELS / MAF_PR_MAX_CLASSES: bounds of maf_pr_match / maf_pr_curves
PR_MAX_LABELS = 1024
PR_MAX_CLASSES = 1024
PR_HEADER = 16                # MAF_PR_HEADER: fp64 summary slots at the start of maf_pr_curves' output
PR_LABELS_XYXY, PR_CONFUSION = 1, 2
PR_ERR_CLASS, PR_ERR_LABELS, PR_ERR_CAPACITY = 1, 2, 4
COCO_T, COCO_R, COCO_A, COCO_M = 10, 101, 4, 3   # MAF_COCO_*: the shape of COCOeval's bbox defaults
COCO_MAX_DETS = 100           # MAF_COCO_MAX_DETS: maxDets[-1], detections kept per (image, category) cell
COCO_MAX_GT = 256             # MAF_COCO_MAX_GT: gts one (image, category) cell may hold
COCO_GT_CROWD, COCO_GT_IDNZ = 1, 2


class MafEmaDesc(C.Structure):
    """maf_ema_desc_t (include/mafyolo_hip.h): one (average, model) tensor pair of maf_ema_update."""
    _fields_ = [("dst", C.c_void_p), ("src", C.c_void_p), ("total", C.c_int64), ("block0", C.c_int32), ("reserved", C.c_int32)]


class MafSgdDesc(C.Structure):
    """maf_sgd_desc_t (include/mafyolo_hip.h): one parameter of maf_sgd_update."""
    _fields_ = [("param", C.c_void_p), ("grad", C.c_void_p), ("buf", C.c_void_p), ("total", C.c_int64), ("block0", C.c_int32), ("group", C.c_int32)]


class MafRangeDesc(C.Structure):
    """maf_range_desc_t (include/mafyolo_hip.h): one contiguous fp32 range of maf_nonfinite_check."""
    _fields_ = [("ptr", C.c_void_p), ("total", C.c_int64), ("block0", C.c_int32), ("reserved", C.c_int32)]


class Phase(int):
    """The `phase` argument of a BatchNorm scratch (csrc/bn_act.hip: which half this call accumulates into) as a step tape sees it: a word that alternates
    from replay to replay (tape.py registers a toggle for the argument slot it is passed in)."""


TAPE_MAX_ARGS = 28


class MafTapeRec(C.Structure):
    """maf_tape_rec_t (include/mafyolo_hip.h): one recorded C-ABI call of a step tape."""
    _fields_ = [("fn", C.c_int32), ("stream", C.c_int32), ("a", C.c_uint64 * TAPE_MAX_ARGS)]


class MafTapeToggle(C.Structure):
    _fields_ = [("addr", C.c_void_p), ("mask", C.c_uint64), ("width", C.c_int32), ("reserved", C.c_int32)]


class MafOp(C.Structure):
    _fields_ = [("kind", C.c_int32), ("dtype", C.c_int32), ("in_dtype", C.c_int32), ("act", C.c_int32),
                ("B", C.c_int32), ("H", C.c_int32), ("W", C.c_int32), ("Hin", C.c_int32), ("Win", C.c_int32),
                ("Cin", C.c_int32), ("Cout", C.c_int32), ("ksize", C.c_int32), ("nsrc", C.c_int32),
                ("src", MafSrc * 4), ("out", C.c_void_p), ("out_stride", C.c_int32), ("out_coff", C.c_int32),
                ("out_f32", C.c_int32), ("tile_p", C.c_int32), ("tile_c", C.c_int32), ("tile_k", C.c_int32),
                ("w", C.c_void_p), ("bias", C.c_void_p),
                ("reg", C.c_void_p * 3), ("lvl_h", C.c_int32 * 3), ("lvl_w", C.c_int32 * 3),
                ("reg_stride", C.c_int32), ("nc", C.c_int32), ("reg_max", C.c_int32), ("lvl_stride", C.c_float * 3),
                ("aux", C.c_void_p * 4), ("lane", C.c_int32), ("n_wait", C.c_int32), ("wait", C.c_int32 * 8),
                ("out_pairs", C.c_int32), ("reserved0", C.c_int32)]


EXPORTS = ["maf_abi_count", "maf_abi_name", "maf_abi_signature", "maf_last_error", "maf_version", "maf_op_size", "maf_op_launch", "maf_engine_create", "maf_engine_num_ops",
           "maf_engine_run", "maf_engine_run_filtered", "maf_engine_run_graph", "maf_engine_run_timed", "maf_engine_destroy", "maf_nms_workspace_bytes", "maf_nms", "maf_nms_ex", "maf_nms_debug", "maf_pack_w1x1_bytes", "maf_pack_w1x1", "maf_pack_dw", "maf_pack_batch", "maf_pack_desc_size", "maf_ema_update", "maf_ema_desc_size", "maf_sgd_update", "maf_sgd_desc_size", "maf_nonfinite_check", "maf_range_desc_size", "maf_maxpool_forward", "maf_maxpool_backward", "maf_upsample2x_forward", "maf_upsample2x_backward", "maf_zero", "maf_grad_fold", "maf_add_sub2", "maf_colsum", "maf_dw_wgrad", "maf_dw_wgrad31", "maf_stem_train", "maf_image_to_nhwc8", "maf_bottleneck_record_bytes", "maf_bottleneck_tail_record_bytes", "maf_bottleneck_tail_supported", "maf_conv1dw_record_bytes", "maf_head_tail_record_bytes", "maf_stem2_record_bytes", "maf_conv3s2_lds_record_bytes", "maf_mprep_lds_record_bytes", "maf_mprep_wreg_record_bytes", "maf_conv3s2_wreg_record_bytes", "maf_conv1x1_stats_supported", "maf_coco_rows", "maf_conv1x1_wgrad", "maf_conv_wgrad", "maf_bn_forward", "maf_bn_backward", "maf_bn_backward_acc", "maf_set_deterministic", "maf_dw_branches", "maf_dw_branches_stats", "maf_bn_forward_ex", "maf_bn_replicas", "maf_bn_stats", "maf_bn_sum_forward", "maf_bn_sum_forward_stats", "maf_bn_sum_backward", "maf_tal_targets", "maf_tal_assign", "maf_atss_assign", "maf_loss_partial_rows", "maf_loss_decode", "maf_loss_terms",
           "maf_detect_join", "maf_detect_join_backward", "maf_nhwc_sum", "maf_stream_fork", "maf_stream_join", "maf_tape_fn_id", "maf_tape_fn_nargs", "maf_tape_rec_size", "maf_tape_run", "maf_tape_toggle",
           "maf_stream_create_masked", "maf_stream_destroy", "maf_letterbox", "maf_letterbox_lds_bytes", "maf_rescale_boxes",
           "maf_augment_resize", "maf_mosaic_affine", "maf_augment_sample_size", "maf_polygon_mask", "maf_mosaic_affine_paste", "maf_augment_paste_size", "maf_area_struct_sizes", "maf_resize_area",
           "maf_pr_state_ints", "maf_pr_out_doubles", "maf_pr_workspace_bytes", "maf_pr_match", "maf_pr_curves",
           "maf_coco_append", "maf_coco_match", "maf_coco_accumulate", "maf_jpeg_struct_sizes", "maf_jpeg_progressive_struct_sizes", "maf_jpeg_decode", "maf_jpeg_encode_struct_sizes", "maf_jpeg_encode", "maf_png_struct_sizes", "maf_png_decode",
           "maf_timer_create", "maf_timer_start", "maf_timer_stop", "maf_timer_elapsed_ms", "maf_timer_destroy"]

_lib = None
_recorder = None              # while a step tape records (tape.py): load() hands out a proxy that notes every tape-able call beside making it


class MafError(RuntimeError):
    pass


def check_sizes(what, have, want, hint=""):
    """The one comparison of what the library says a struct measures (`have`: a size or a list of sizes) with what this binding declares."""
    if have != want:
        raise MafError("libmafyolo_hip.so was built for %s of %s bytes, this binding declares %s: rebuild%s" % (what, have, want, hint))


# a character of a signature of the library's table (include/mafyolo_hip.h, maf_abi_signature) -> the ctypes type that passes it
ABI_KINDS = {"v": None, "s": C.c_char_p, "p": C.c_void_p, "f": C.c_float, "d": C.c_double, "i": C.c_int32, "l": C.c_int64}
# Pointer parameters that ctypes is to type-check and convert (a structure passed by reference, an array, None) instead of taking an address: function ->
# {slot: type}.  The only thing about a signature that is written here; everything else comes from the library.
_INT32_OUT = {0: C.POINTER(C.c_int32)}
TYPED_POINTERS = {
    "maf_op_launch": {0: C.POINTER(MafOp)},
    "maf_engine_create": {0: C.POINTER(MafOp), 2: C.POINTER(C.c_void_p)},
    "maf_engine_run_timed": {4: C.POINTER(C.c_float)},
    "maf_nms_debug": {0: C.POINTER(C.c_uint64)},
    "maf_sgd_update": {4: C.POINTER(C.c_double), 5: C.POINTER(C.c_double), 6: C.POINTER(C.c_double), 7: C.POINTER(C.c_int32)},
    "maf_stream_create_masked": {2: C.POINTER(C.c_void_p)},
    "maf_tape_run": {5: C.POINTER(C.c_int32)},
    "maf_letterbox": {0: C.POINTER(MafLetterboxImage), 5: C.POINTER(C.c_uint8)},
    "maf_letterbox_lds_bytes": {0: C.POINTER(MafLetterboxImage)},
    "maf_area_struct_sizes": _INT32_OUT, "maf_jpeg_struct_sizes": _INT32_OUT, "maf_jpeg_progressive_struct_sizes": _INT32_OUT,
    "maf_jpeg_encode_struct_sizes": _INT32_OUT, "maf_png_struct_sizes": _INT32_OUT,
    "maf_timer_create": {0: C.POINTER(C.c_void_p)},
    "maf_timer_elapsed_ms": {1: C.POINTER(C.c_float)},
}


def bind(lib):
    """Set restype and argtypes of every exported function from the signature table inside the library (csrc/abi.hip: derived from the header's
    prototypes by the compiler), with the pointers of TYPED_POINTERS refined."""
    if not hasattr(lib, "maf_abi_count"):
        raise MafError("libmafyolo_hip.so has no signature table (maf_abi_count): it was built before this binding took its types from the library: rebuild "
                       "(__graft_entry__.build())")
    lib.maf_abi_count.restype, lib.maf_abi_count.argtypes = C.c_int32, []
    for fn in (lib.maf_abi_name, lib.maf_abi_signature):
        fn.restype, fn.argtypes = C.c_char_p, [C.c_int32]
    table = {lib.maf_abi_name(i).decode(): lib.maf_abi_signature(i).decode() for i in range(lib.maf_abi_count())}
    odd = sorted((set(table) ^ set(EXPORTS)) | (set(TYPED_POINTERS) - set(table)))
    if odd:
        raise MafError("libmafyolo_hip.so's signature table, lib.EXPORTS and lib.TYPED_POINTERS do not name the same functions: %s: rebuild, or bring "
                       "csrc/abi.hip and lib.py in line with include/mafyolo_hip.h" % ", ".join(odd))
    for name, sig in table.items():
        ret, params = sig.split(":")
        types = [ABI_KINDS[k] for k in params]
        for slot, typ in TYPED_POINTERS.get(name, {}).items():
            if slot >= len(params) or params[slot] != "p":
                raise MafError("lib.TYPED_POINTERS types argument %d of %s, which the library declares as '%s' (no pointer there)" % (slot, name, sig))
            types[slot] = typ
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = ABI_KINDS[ret], types


def load():
    """Load the HIP library (once). Raises MafError if it has not been built (run __graft_entry__.build())."""
    global _lib
    if _recorder is not None:
        return _recorder
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise MafError("libmafyolo_hip.so not found at %s — the HIP extension is not built; "
                       "run `python -c 'import __graft_entry__ as g; g.build()'` (there is no CPU fallback)" % LIB_PATH)
    lib = C.CDLL(LIB_PATH)
    bind(lib)
    check_sizes("a maf_op_t", lib.maf_op_size(), C.sizeof(MafOp), " (__graft_entry__.build())")
    check_sizes("a maf_tape_rec_t", lib.maf_tape_rec_size(), C.sizeof(MafTapeRec))
    check_sizes("a maf_augment_paste_t", lib.maf_augment_paste_size(), C.sizeof(MafAugmentPaste))
    check_sizes("a maf_augment_sample_t", lib.maf_augment_sample_size(), C.sizeof(MafAugmentSample))
    _lib = lib
    return lib


def check(rc):
    if rc != 0:
        raise MafError("libmafyolo_hip: %s (code %d)" % (load().maf_last_error().decode(), rc))


class Timer:
    """HIP events recorded on an explicit stream (torch.cuda.Event only sees torch's current stream)."""

    def __init__(self):
        self._h = C.c_void_p()
        check(load().maf_timer_create(C.byref(self._h)))

    def start(self, stream):
        check(load().maf_timer_start(self._h, stream))

    def stop(self, stream):
        check(load().maf_timer_stop(self._h, stream))

    def elapsed_ms(self):
        ms = C.c_float()
        check(load().maf_timer_elapsed_ms(self._h, C.byref(ms)))
        return ms.value

    def __del__(self):
        try:
            if self._h:
                load().maf_timer_destroy(self._h)
        except Exception:
            pass
