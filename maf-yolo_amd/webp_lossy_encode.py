"""Frames in, file bytes out, on the device: lossy WebP (one VP8 key frame) files that libwebp and this project's webp_lossy.decode return to the
same frame.

What people do with a detector's output at scale, cv2.imwrite(path, img, [cv2.IMWRITE_WEBP_QUALITY, q]) for millions of save_one_box crops and
annotated frames (the lossy `VP8 ` chunk), without a device -> host copy per frame and libwebp on one core:
  * encode(frames, ...)     a list of uint8 [h, w, 3] BGR CUDA tensors (or one [B, h, w, 3]), optionally rectangles of them (jpeg_encode.crop_rects
                            gives save_one_box's) -> jpeg_encode.EncodedBatch: ONE pinned staging buffer, ONE host -> device copy, five launches
                            and one memset for the whole call whatever it holds (csrc/vp8_encode.hip), no host synchronisation;
  * EncodedBatch.files()    -> list[bytes]; the only call that synchronises.
What is written (the "profile", restated rule by rule in tests/webp_lossy_encode_ref.py, whose bytes the device equals): RIFF / WEBP with ONE
`VP8 ` chunk, no VP8X and no metadata; one visible key frame, version 0, no scaling; no segments, no loop-filter deltas, sharpness 0, the normal
filter at `filter_level`, all five dq 0.  BGR -> Y, U, V by integer BT.601 with the chroma taken from the plain sum of each 2x2 block (this
project's rule: libwebp's gamma-aware averaging is not restated and no identity with its converter is claimed); odd sizes and the padding to
whole macroblocks replicate the last column and row.  Every macroblock is predicted 16x16: the luma mode is the one of DC, TM, V, H with the
lowest sum of squared differences between the source and the prediction from the RECONSTRUCTED neighbours (ties: the lowest number), the chroma
mode likewise over U and V together.  libwebp's integer forward DCT and WHT; level = sign(c) * min((|c| + (q >> 1)) // q, 2047); the
reconstruction goes through the decoder's dequantiser and inverse transforms, so the next macroblock predicts from what a decoder will see.  A
macroblock without a level is a skip when skip_proba = (total - skips) * 255 // total is below 250 (else use_skip = 0).  Default coefficient
probabilities, no updates.  2^log2_parts token partitions, log2_parts = min(argument, floor(log2(macroblock rows))): libwebp refuses a file
whose last partition is empty.

Quality: `base_q` (0 .. 127, the frame's quantiser index) wins when given; otherwise `quality` (0 .. 100) maps by libwebp's curve
c = q / 100; c = 2c / 3 if c < 0.75 else 2c - 1; base_q = int(127 * (1 - c ** (1 / 3))).  That is NOT the index Pillow's files carry, because
libwebp then applies its segment and SNS adjustments; on a 96 x 64 test frame, read back with webp_lossy_ref.describe:
    quality          10   50   75   90  100
    Pillow's base_q  92   52   36   12    0
    this mapping     75   38   26    9    0

What is claimed: the files are legal VP8, libwebp (Pillow) and webp_lossy.decode return the same frame from them, and the bytes are the rule
book's.  cv2.imwrite's own bytes are UNCHECKED and NOT claimed.  No CPU fallback.

Bounds.  A bool costs as many bits as its renormalisation shifts, at most 7.  The first partition holds 1094 bools in front of the modes and at
most 8 per macroblock; taken at 8 bits each that is 1094 + 8 * macroblocks + 4 flush bytes, which must stay below the 2^19 of the frame tag's
size field: at most 65 398 macroblocks per file (16.7 megapixels).  The tokens of one macroblock take at most MB_BITS = 20 675 bits: per
(type, band, context) the dearest path through the token tree under the default probabilities, each bool at its worst shift count over every
range 128 .. 255, the extra bits at their table probabilities, the sign at 1 bit (webp_lossy_encode_ref.mb_worst_bits derives the number and the
host test compares).  That is 2 585 bytes per macroblock, 6.7 per pixel, held once in the partition buffers and once in the output: 3.0 MiB per
640 x 480 frame each, 189 MiB in all for 32 such frames (levels, planes and reconstruction add 1.8 MiB per frame).
Not done: 4x4 prediction and the i4 / i16 decision; segments and coefficient-probability updates; rate control, or byte parity with libwebp's
encoder (impossible: its output follows heuristics); alpha, VP8X and metadata.
"""
import ctypes as C

import numpy as np

from . import lib, staging
from .jpeg_encode import EncodedBatch
from .lib import MafError

MAX_SIDE = 16383              # MAF_VP8_ENC_MAX_SIDE
FILE_BYTES = 20               # MAF_VP8_ENC_FILE_BYTES: RIFF, size, WEBP, `VP8 `, size
FRAME_BYTES = 10              # MAF_VP8_ENC_FRAME_BYTES
HEADER_BOOLS = 1094           # MAF_VP8_ENC_HEADER_BOOLS
MODE_BOOLS = 8                # MAF_VP8_ENC_MODE_BOOLS
FLUSH_BYTES = 4               # MAF_VP8_ENC_FLUSH_BYTES
MB_BITS = 20675               # MAF_VP8_ENC_MB_BITS
MB_LEVELS = 400               # MAF_VP8_ENC_MB_LEVELS
META_WORDS = 16               # MAF_VP8_ENC_META_WORDS
MAX_P0 = 1 << 19              # MAF_VP8_ENC_MAX_P0
MAX_MBS = (MAX_P0 - 1 - HEADER_BOOLS - FLUSH_BYTES) // MODE_BOOLS      # 65398

HEADER_DT = np.dtype([("n_files", "<i4"), ("base_q", "<i4"), ("level", "<i4"), ("max_chroma", "<i4"), ("jobs_off", "<i8"), ("total_bytes", "<i8"),
                      ("plane_bytes", "<i8"), ("n_mbs", "<i8"), ("part_bytes", "<i8"), ("out_bytes", "<i8")])   # maf_vp8_enc_header_t
JOB_DT = np.dtype([("src", "<u8"), ("pitch", "<i8"), ("plane_off", "<i8"), ("part_off", "<i8"), ("part_bytes", "<i8"), ("mb0", "<i8"), ("w", "<i4"),
                   ("h", "<i4"), ("mbw", "<i4"), ("mbh", "<i4"), ("log2_parts", "<i4"), ("reserved", "<i4")])   # maf_vp8_enc_job_t

# AC_Q of the format (csrc/vp8_tables.h k_vp8_ac_q), for the default filter level
_AC_Q = (list(range(4, 59)) + list(range(60, 118, 2)) + list(range(119, 176, 3)) + list(range(177, 233, 4)) +
         [234, 239, 245, 249, 254, 259, 264, 269, 274, 279, 284])


def quality_to_base_q(quality):
    """libwebp's curve from quality 0 .. 100 to the quantiser index (the table in the module docstring)."""
    c = quality / 100.0
    c = 2.0 * c / 3.0 if c < 0.75 else 2.0 * c - 1.0
    return int(127.0 * (1.0 - c ** (1.0 / 3.0)))


def default_filter_level(base_q):
    """min(63, AC_Q[base_q] >> 2): the loop filter's level where none is given."""
    return min(63, _AC_Q[base_q] >> 2)


def _first_bound(n_mbs):
    """Bytes the first partition of a file of `n_mbs` macroblocks can take (MAF_VP8_ENC_P0_BOUND): 1094 header bools and at most 8 per
    macroblock, at most 8 bits each, and the coder's 4 flush bytes."""
    return HEADER_BOOLS + MODE_BOOLS * n_mbs + FLUSH_BYTES


def _part_bound(n_mbs):
    """Bytes a token partition of `n_mbs` macroblocks can take (MAF_VP8_ENC_PART_BOUND): MB_BITS bits each, and the 4 flush bytes."""
    return (MB_BITS * n_mbs + 7) // 8 + FLUSH_BYTES


def _worst_case_bytes(mbw, mbh, log2_parts):
    """-> (bytes of a file's partitions, bytes of the file) at the most: token partition p of n owns the macroblock rows p, p + n, ..."""
    n = 1 << log2_parts
    parts = _first_bound(mbw * mbh) + sum(_part_bound(mbw * ((mbh - p + n - 1) // n)) for p in range(n))
    return parts, FILE_BYTES + FRAME_BYTES + parts + 3 * (n - 1) + 1


# the hand-written binding of include/mafyolo_vp8_encode.h (tests/test_webp_lossy_encode_host.py compares the two)
PROTOTYPES = {
    "maf_vp8_encode_struct_sizes": (C.c_int32, [C.POINTER(C.c_int32)]),
    "maf_vp8_encode": (C.c_int32, [C.c_void_p] * 12),
}
_bound = False


def _bind(L):
    """Set restype and argtypes of the two entry points on the handle lib.load() returns; a library without them is an error."""
    global _bound
    for name, (res, args) in PROTOTYPES.items():
        if not hasattr(L, name):
            raise MafError("libmafyolo_hip.so lacks %s (csrc/vp8_encode.hip): rebuild (__graft_entry__.build())" % name)
        fn = getattr(L, name)
        fn.restype, fn.argtypes = res, args
    _bound = True
    return L


def _library():
    L = lib.load()
    if not _bound:
        _bind(L)
    return staging.checked_library("webp_lossy_encode", (("maf_vp8_encode_struct_sizes", 2),), [HEADER_DT.itemsize, JOB_DT.itemsize], "maf_vp8_enc_* structs")


_FRAME_TEXT = {      # staging.frame_list in encode()'s words
    "batch": "webp_lossy_encode.encode: a tensor of frames is [B, h, w, 3], got %(shape)s",
    "none": "webp_lossy_encode.encode: no frames",
    "not_tensor": "webp_lossy_encode.encode: frame %(i)d is a %(kind)s, not a CUDA tensor",
    "cpu": "webp_lossy_encode.encode runs on the HIP path only (no CPU fallback): frame %(i)d is on %(device)s",
    "device": "webp_lossy_encode.encode: frame %(i)d is on %(device)s, frame 0 on %(first)s",
    "type": "webp_lossy_encode.encode: frame %(i)d must be uint8 [h, w, 3] BGR, got %(dtype)s %(shape)s",
    "empty": "webp_lossy_encode.encode: frame %(i)d is empty (%(w)d x %(h)d): there is no WebP file of an empty image",
    "too_large": "webp_lossy_encode.encode: frame %(i)d is %(w)d x %(h)d, a side is at most 65535",
    "stride": "webp_lossy_encode.encode: frame %(i)d must have pixel stride 3 and channel stride 1 (any row pitch of at least 3 * w), got strides %(strides)s"}
_FRAME_TEXT["pitch"] = _FRAME_TEXT["stride"]


def _int_in(name, v, lo, hi):
    if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not lo <= v <= hi:
        raise MafError("webp_lossy_encode.encode: %s is an int from %d to %d, got %r" % (name, lo, hi, v))
    return int(v)


def encode(frames, quality=75, base_q=None, filter_level=None, log2_parts=3, rects=None, stream=None, taps=None):
    """Encode frames (a list of uint8 [h, w, 3] BGR CUDA tensors of any sizes, or one [B, h, w, 3] tensor; pixel stride 3, channel stride 1, any row
    pitch: read in place) to lossy WebP files on the device -> EncodedBatch.  `quality`: 0 .. 100, mapped by quality_to_base_q; `base_q`: 0 .. 127,
    the quantiser index itself, wins when given.  `filter_level`: 0 .. 63, None: default_filter_level(base_q).  `log2_parts`: 0 .. 3, a file has
    min(2^log2_parts, 2^floor(log2(macroblock rows))) token partitions.  `rects`: a host int array [R, 5] of (frame index, x1, y1, x2, y2): one file
    per rectangle frame[y1:y2, x1:x2] instead of one per frame; a file's side is at most 16383 and it has at most 65398 macroblocks.  `stream`: a
    torch.cuda.Stream to work on (default: the current one).  Every buffer is sized on the host from _worst_case_bytes, so nothing is read back
    here.  `taps`: a dict that receives the intermediate buffers (planes: the Y, U, V that went in; recon: the unfiltered reconstruction; levels;
    info: modes, non-zero and skip flags; meta: skipped macroblocks, status, partition sizes; parts; the job table, the header) — tests and the probe."""
    import torch
    if base_q is None:
        if isinstance(quality, bool) or not isinstance(quality, (int, float, np.integer, np.floating)) or not 0 <= quality <= 100:
            raise MafError("webp_lossy_encode.encode: quality is a number from 0 to 100, got %r" % (quality,))
        base_q = quality_to_base_q(float(quality))
    base_q = _int_in("base_q", base_q, 0, 127)
    level = default_filter_level(base_q) if filter_level is None else _int_in("filter_level", filter_level, 0, 63)
    log2_parts = _int_in("log2_parts", log2_parts, 0, 3)
    frames = staging.frame_list(frames, _FRAME_TEXT)
    fi, x1, y1, x2, y2 = staging.rect_list(frames, rects, "webp_lossy_encode.encode", "WebP")
    fw = np.array([f.shape[1] for f in frames], np.int64)
    n = len(fi)
    if n > staging.MAX_FILES:
        raise MafError("webp_lossy_encode.encode takes up to 65535 files per call")
    w, h = x2 - x1, y2 - y1
    side = np.maximum(w, h)
    if side.max() > MAX_SIDE:
        k = int(side.argmax())
        raise MafError("webp_lossy_encode.encode: file %d is %d x %d, a side is at most 16383 (the format's 14 bits)" % (k, w[k], h[k]))
    mbw, mbh = (w + 15) >> 4, (h + 15) >> 4
    nmb = mbw * mbh
    if nmb.max() > MAX_MBS:
        k = int(nmb.argmax())
        raise MafError("webp_lossy_encode.encode: file %d is %d x %d, %d macroblocks: at most %d are taken (the first partition's worst case, 1094 + 8 per "
                       "macroblock + 4 bytes, must stay below the 2^19 of the frame tag's size field)" % (k, w[k], h[k], nmb[k], MAX_MBS))
    lp = np.minimum(log2_parts, np.floor(np.log2(mbh)).astype(np.int64))     # every partition owns a macroblock row
    bounds = [_worst_case_bytes(int(a), int(b), int(c)) for a, b, c in zip(mbw, mbh, lp)]
    part_size = staging.align(np.array([b[0] for b in bounds], np.int64))
    out_bytes = int(sum(b[1] for b in bounds))
    plane = 384 * nmb
    pitch = np.maximum(np.array([f.stride(0) for f in frames], np.int64), 3 * fw)[fi]      # a one-row frame may carry any stride 0: it is never used
    base = np.array([f.data_ptr() for f in frames], np.uint64)[fi]
    jobs = np.zeros(n, JOB_DT)
    jobs["src"] = base + (y1 * pitch + 3 * x1).astype(np.uint64)
    jobs["pitch"], jobs["w"], jobs["h"], jobs["mbw"], jobs["mbh"], jobs["log2_parts"] = pitch, w, h, mbw, mbh, lp
    jobs["plane_off"], jobs["mb0"] = np.cumsum(plane) - plane, np.cumsum(nmb) - nmb
    jobs["part_off"], jobs["part_bytes"] = np.cumsum(part_size) - part_size, part_size
    plane_bytes, n_mbs, part_bytes = int(plane.sum()), int(nmb.sum()), int(part_size.sum())
    sections = (("jobs_off", jobs),)
    hdr, off = staging.blob_layout(HEADER_DT, sections)
    hdr["n_files"], hdr["base_q"], hdr["level"], hdr["max_chroma"], hdr["total_bytes"] = n, base_q, level, 64 * int(nmb.max()), off
    hdr["plane_bytes"], hdr["n_mbs"], hdr["part_bytes"], hdr["out_bytes"] = plane_bytes, n_mbs, part_bytes, out_bytes
    if off >= staging.MAX_BLOB:
        raise MafError("webp_lossy_encode.encode: the job table of one call is limited to 2 GiB")
    L = _library()
    dev = frames[0].device
    if stream is not None:
        for f in frames:
            f.record_stream(stream)                                          # the allocator must not hand a dropped frame on while `stream` still reads it
    with staging.staged(off, dev, stream, zeros=True) as s:                  # zeros: the alignment gaps are defined bytes
        staging.write_blob(s.host, hdr, sections)
        blob = s.copy()
        planes = torch.empty(plane_bytes, dtype=torch.uint8, device=dev)
        recon = torch.empty(plane_bytes, dtype=torch.uint8, device=dev)
        levels = torch.empty(MB_LEVELS * n_mbs, dtype=torch.int16, device=dev)
        info = torch.empty(n_mbs, dtype=torch.int32, device=dev)
        meta = torch.empty(META_WORDS * n, dtype=torch.int32, device=dev)    # zeroed by the library on the stream
        parts = torch.empty(part_bytes, dtype=torch.uint8, device=dev)
        out = torch.empty(out_bytes, dtype=torch.uint8, device=dev)          # the files are written back to back
        lengths = torch.empty(n, dtype=torch.int32, device=dev)
        offsets = torch.empty(n, dtype=torch.int64, device=dev)
        lib.check(L.maf_vp8_encode(s.host.ctypes.data, blob.data_ptr(), planes.data_ptr(), recon.data_ptr(), levels.data_ptr(), info.data_ptr(), meta.data_ptr(),
                                   parts.data_ptr(), out.data_ptr(), lengths.data_ptr(), offsets.data_ptr(), s.stream.cuda_stream))
    if taps is not None:
        taps.update(planes=planes, recon=recon, levels=levels, info=info, meta=meta, parts=parts, jobs=jobs, header=hdr)
    return EncodedBatch(out, offsets, lengths, s.stream, (frames, s.pinned, blob, planes, recon, levels, info, meta, parts))
