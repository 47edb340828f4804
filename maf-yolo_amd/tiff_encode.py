"""Frames in, file bytes out, on the device: TIFF encoding whose strips equal, byte for byte, what libtiff writes at cv2.imwrite's settings.

The last step of the reference's tools/infer.py for a .tif / .tiff source, which it runs on the host one picture at a time:
cv2.imwrite(save_path, img_src), where save_path keeps the source file's name and so its extension (yolov6/core/inferer.py):
  * encode(frames, ...)     a list of uint8 [h, w, 3] BGR CUDA tensors (or one [B, h, w, 3]), optionally rectangles of them (jpeg_encode.crop_rects
                            gives save_one_box's) -> jpeg_encode.EncodedBatch: ONE pinned staging buffer, ONE host -> device copy, one memset and
                            six launches for the whole call whatever it holds (csrc/tiff_encode.hip), no host synchronisation;
  * EncodedBatch.files()    -> list[bytes]; the only call that synchronises.
What is written: a little-endian classic TIFF, 8-bit RGB (Photometric 2, PlanarConfiguration 1), strips of RowsPerStrip rows compressed with
LZW (Compression 5) over rows differenced horizontally (Predictor 2; predictor=False writes the plain rows and no Predictor tag).  Every
strip's bytes are exactly what libtiff 4.7.1 writes for the same rows at the same settings, and the tag values are libtiff's.  The file around
the strips is ours: the header, the strips back to back from byte 8, a pad byte where they end at an odd offset, the BitsPerSample,
StripOffsets and StripByteCounts arrays, then the IFD (eleven entries in ascending tag order, ten without the predictor; SHORT but for the two
LONG strip arrays, which hold their value inline for a single strip; next-IFD 0).  The rules are restated in tests/tiff_encode_ref.py and
pinned there to Pillow / libtiff.

cv2.imwrite itself — UNCHECKED, OpenCV is not installed where this was written.  It hands libtiff Compression 5, Predictor 2,
PlanarConfiguration 1, Photometric 2 and RowsPerStrip = clamp(8192 // (3 * w), 1, h), the division first, and those are the settings pinned
here (rows_per_strip=None); so the pixels and the strips should be cv2's.  Byte identity of the FILE with cv2.imwrite is NOT claimed and
nobody checks it.  Parity is claimed with libtiff's strips only.  No CPU fallback.
The output buffer is sized from _worst_case_bytes.
Not done: gray, palette, alpha and 16-bit output; tiles; other compressions; BigTIFF; big-endian files; resolution and software tags.
"""
import ctypes as C

import numpy as np

from . import lib, staging
from .jpeg_encode import EncodedBatch
from .lib import MafError

CHUNK = 4096                  # MAF_TIFF_ENC_CHUNK
TABLE = 8192                  # MAF_TIFF_ENC_TABLE
MAX_STRIP = 1 << 23           # MAF_TIFF_ENC_MAX_STRIP: bytes of one strip, exclusive
MAX_FILE = 1 << 31            # MAF_TIFF_ENC_MAX_FILE: worst-case bytes of one file, exclusive
MAX_SIDE = 65535

HEADER_DT = np.dtype([("n_files", "<i4"), ("n_strips", "<i4"), ("n_chunks", "<i4"), ("reserved", "<i4"), ("jobs_off", "<i8"), ("total_bytes", "<i8"),
                      ("raw_bytes", "<i8"), ("code_elems", "<i8"), ("out_bytes", "<i8")])   # maf_tiff_enc_header_t
JOB_DT = np.dtype([("src", "<u8"), ("pitch", "<i8"), ("raw_off", "<i8"), ("code_off", "<i8"), ("w", "<i4"), ("h", "<i4"), ("rows_per_strip", "<i4"),
                   ("predictor", "<i4"), ("strip0", "<i4"), ("n_strips", "<i4"), ("chunk0", "<i4"), ("n_chunks", "<i4"), ("code_slot", "<i4"),
                   ("reserved", "<i4")])   # maf_tiff_enc_job_t
STRIP_DT = np.dtype([("n_codes", "<i4"), ("bits", "<i4"), ("offset", "<u4"), ("bytes", "<u4")])   # maf_tiff_enc_strip_t


def cv2_rows_per_strip(w, h):
    """RowsPerStrip as cv2.imwrite sets it (as remembered, see the module docstring): clamp(8192 // (3 * w), 1, h)."""
    return np.minimum(np.maximum(8192 // (3 * np.asarray(w, np.int64)), 1), h)


def _worst_case_codes(n):
    """Codes the LZW stream of a strip of `n` bytes can hold (MAF_TIFF_ENC_CODE_BOUND), the size of a strip's slot in the code buffer: at most n
    data codes, n // 3836 Clears of a full table, n // 10000 Clears at ratio checkpoints, the Clear in front and the EOI (derived in
    _worst_case_bytes)."""
    return n + n // 3836 + n // 10000 + 2


def _worst_case_bytes(n):
    """Bytes the LZW stream of a strip of `n` bytes can take (MAF_TIFF_ENC_BYTE_BOUND): ceil(12 * (n + n // 3836 + n // 10000 + 2) / 8), about
    1.5 n.  Derived from the rule (tests/tiff_encode_ref.py lzw), code by code: a data code is written only when an input byte ends a match,
    and once more at the strip's end, so there are at most n; a Clear stands in front (1); a Clear is written when the table is full, which
    takes 3836 data codes since the Clear before (at most n // 3836, the one behind the last data code included); a Clear is written at a
    ratio checkpoint at the most, and checkpoints lie at least 10000 input bytes apart, because a reset zeroes the input count and keeps the
    checkpoint (at most n // 10000); the EOI is 1.  That is _worst_case_codes(n) codes; none is wider than 12 bits, and the zero bits that
    pad the last byte round the sum up to whole bytes.  Noise takes about 1.37 n (tests/test_tiff_encode_host.py)."""
    return (12 * _worst_case_codes(n) + 7) // 8


def _tail_bytes(n_strips, predictor):
    """Bytes of a file behind its strips and the pad byte: BitsPerSample, the two strip arrays (inline for one strip), the IFD."""
    return 6 + np.where(n_strips > 1, 8 * n_strips, 0) + 2 + 12 * (11 if predictor else 10) + 4


# the hand-written binding of include/mafyolo_tiff_encode.h (tests/test_tiff_encode_host.py compares the two)
PROTOTYPES = {
    "maf_tiff_encode_struct_sizes": (C.c_int32, [C.POINTER(C.c_int32)]),
    "maf_tiff_encode": (C.c_int32, [C.c_void_p] * 9),
}
_bound = False


def _bind(L):
    """Set restype and argtypes of the two entry points on the handle lib.load() returns; a library without them is an error."""
    global _bound
    for name, (res, args) in PROTOTYPES.items():
        if not hasattr(L, name):
            raise MafError("libmafyolo_hip.so lacks %s (csrc/tiff_encode.hip): rebuild (__graft_entry__.build())" % name)
        fn = getattr(L, name)
        fn.restype, fn.argtypes = res, args
    _bound = True
    return L


def _library():
    L = lib.load()
    if not _bound:
        _bind(L)
    return staging.checked_library("tiff_encode", (("maf_tiff_encode_struct_sizes", 3),), [HEADER_DT.itemsize, JOB_DT.itemsize, STRIP_DT.itemsize],
                                   "maf_tiff_enc_* structs")


_FRAME_TEXT = {      # staging.frame_list in encode()'s words
    "batch": "tiff_encode.encode: a tensor of frames is [B, h, w, 3], got %(shape)s",
    "none": "tiff_encode.encode: no frames",
    "not_tensor": "tiff_encode.encode: frame %(i)d is a %(kind)s, not a CUDA tensor",
    "cpu": "tiff_encode.encode runs on the HIP path only (no CPU fallback): frame %(i)d is on %(device)s",
    "device": "tiff_encode.encode: frame %(i)d is on %(device)s, frame 0 on %(first)s",
    "type": "tiff_encode.encode: frame %(i)d must be uint8 [h, w, 3] BGR, got %(dtype)s %(shape)s",
    "empty": "tiff_encode.encode: frame %(i)d is empty (%(w)d x %(h)d): there is no TIFF file of an empty image",
    "too_large": "tiff_encode.encode: frame %(i)d is %(w)d x %(h)d, a side is at most 65535 (tiff_encode.MAX_SIDE)",
    "stride": "tiff_encode.encode: frame %(i)d must have pixel stride 3 and channel stride 1 (any row pitch of at least 3 * w), got strides %(strides)s"}
_FRAME_TEXT["pitch"] = _FRAME_TEXT["stride"]


def encode(frames, rects=None, rows_per_strip=None, predictor=True, stream=None, taps=None):
    """Encode frames (a list of uint8 [h, w, 3] BGR CUDA tensors of any sizes, or one [B, h, w, 3] tensor; pixel stride 3, channel stride 1, any row
    pitch: read in place) to TIFF files on the device -> EncodedBatch.  `rects`: a host int array [R, 5] of (frame index, x1, y1, x2, y2): one
    file per rectangle frame[y1:y2, x1:x2] (jpeg_encode.crop_rects gives save_one_box's) instead of one per frame.  `rows_per_strip`: None
    for cv2.imwrite's clamp(8192 // (3 * w), 1, h) per file, or an integer from 1 to h for every file, or one such integer per file.
    `predictor`: True differences the rows (Predictor 2, cv2.imwrite's), False writes them as they are and no Predictor tag.  `stream`: a
    torch.cuda.Stream to work on (default: the current one).  Every buffer is sized on the host from _worst_case_bytes, so nothing is read
    back here.  `taps`: a dict that receives the intermediate buffers (raw, codes, strips, the job table, the header) — tests and the probe."""
    import torch
    frames = staging.frame_list(frames, _FRAME_TEXT)
    fi, x1, y1, x2, y2 = staging.rect_list(frames, rects, "tiff_encode.encode", "TIFF")
    fw = np.array([f.shape[1] for f in frames], np.int64)
    n = len(fi)
    if n > staging.MAX_FILES:
        raise MafError("tiff_encode.encode takes up to 65535 files per call")
    w, h = x2 - x1, y2 - y1
    if rows_per_strip is None:
        rps = cv2_rows_per_strip(w, h)
    else:
        given = np.asarray(rows_per_strip)
        if given.dtype.kind not in "iu" or given.shape not in ((), (n,)):
            raise MafError("tiff_encode.encode: rows_per_strip is None (cv2.imwrite's rule), an integer from 1 to h or one such integer per file, got %r"
                           % (rows_per_strip,))
        rps = np.broadcast_to(given.astype(np.int64), (n,))
        bad = np.flatnonzero((rps < 1) | (rps > h))
        if bad.size:
            k = int(bad[0])
            raise MafError("tiff_encode.encode: rows_per_strip %d is outside 1..h for file %d (%d x %d)" % (rps[k], k, w[k], h[k]))
    full = 3 * w * rps                                                        # bytes of a strip that is not the last
    if full.max() >= MAX_STRIP:
        k = int(full.argmax())
        raise MafError("tiff_encode.encode: file %d (%d x %d) has strips of %d bytes (%d rows), fewer than 8 MiB are taken: lower rows_per_strip"
                       % (k, w[k], h[k], full[k], rps[k]))
    ns = -(-h // rps)
    n_raw = 3 * w * h
    last = n_raw - (ns - 1) * full
    bound = 8 + (ns - 1) * _worst_case_bytes(full) + _worst_case_bytes(last) + 1 + _tail_bytes(ns, predictor)      # per file: header, strips, pad byte, tail
    if bound.max() >= MAX_FILE:
        k = int(bound.argmax())
        raise MafError("tiff_encode.encode: file %d (%d x %d) can take %d bytes, fewer than 2 GiB are taken (BigTIFF is not done)" % (k, w[k], h[k], bound[k]))
    pitch = np.maximum(np.array([f.stride(0) for f in frames], np.int64), 3 * fw)[fi]      # a one-row frame may carry any stride 0: it is never used
    base = np.array([f.data_ptr() for f in frames], np.uint64)[fi]
    raw_size = staging.align(n_raw)
    nc = -(-n_raw // CHUNK)
    slot = _worst_case_codes(full)
    jobs = np.zeros(n, JOB_DT)
    jobs["src"] = base + (y1 * pitch + 3 * x1).astype(np.uint64)
    jobs["pitch"], jobs["w"], jobs["h"], jobs["rows_per_strip"], jobs["predictor"] = pitch, w, h, rps, 1 if predictor else 0
    jobs["raw_off"], jobs["code_off"], jobs["code_slot"] = np.cumsum(raw_size) - raw_size, np.cumsum(ns * slot) - ns * slot, slot
    jobs["strip0"], jobs["n_strips"] = np.cumsum(ns) - ns, ns
    jobs["chunk0"], jobs["n_chunks"] = np.cumsum(nc) - nc, nc
    raw_bytes, code_elems, strips, chunks = int(raw_size.sum()), int((ns * slot).sum()), int(ns.sum()), int(nc.sum())
    out_bytes = staging.align(int(bound.sum()), 4)
    if strips >= 1 << 30 or chunks >= 1 << 30:
        raise MafError("tiff_encode.encode: %d strips in one call, fewer than 2^30 are taken (split the batch)" % strips)
    sections = (("jobs_off", jobs),)
    hdr, off = staging.blob_layout(HEADER_DT, sections)
    hdr["n_files"], hdr["n_strips"], hdr["n_chunks"], hdr["total_bytes"] = n, strips, chunks, off
    hdr["raw_bytes"], hdr["code_elems"], hdr["out_bytes"] = raw_bytes, code_elems, out_bytes
    if off >= staging.MAX_BLOB:
        raise MafError("tiff_encode.encode: the job table of one call is limited to 2 GiB")
    L = _library()
    dev = frames[0].device
    if stream is not None:
        for f in frames:
            f.record_stream(stream)                                          # the allocator must not hand a dropped frame on while `stream` still reads it
    with staging.staged(off, dev, stream, zeros=True) as s:                  # zeros: the alignment gaps are defined bytes
        staging.write_blob(s.host, hdr, sections)
        blob = s.copy()
        raw = torch.empty(raw_bytes, dtype=torch.uint8, device=dev)
        codes = torch.empty(code_elems, dtype=torch.int16, device=dev)       # uint16 on the device
        table = torch.empty(strips * STRIP_DT.itemsize, dtype=torch.uint8, device=dev)
        out = torch.empty(out_bytes, dtype=torch.uint8, device=dev)          # zeroed by the library on the stream; the files are written back to back
        lengths = torch.empty(n, dtype=torch.int32, device=dev)
        offsets = torch.empty(n, dtype=torch.int64, device=dev)
        lib.check(L.maf_tiff_encode(s.host.ctypes.data, blob.data_ptr(), raw.data_ptr(), codes.data_ptr(), table.data_ptr(), out.data_ptr(),
                                    lengths.data_ptr(), offsets.data_ptr(), s.stream.cuda_stream))
    if taps is not None:
        taps.update(raw=raw, codes=codes, strips=table, jobs=jobs, header=hdr)
    return EncodedBatch(out, offsets, lengths, s.stream, (frames, s.pinned, blob, raw, codes, table))
