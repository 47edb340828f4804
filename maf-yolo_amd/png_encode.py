"""Frames in, file bytes out, on the device: PNG encoding whose zlib stream equals, byte for byte, what zlib writes at cv2.imwrite's settings.

The last step of the reference's tools/infer.py for a .png source, which it runs on the host one picture at a time: cv2.imwrite(save_path,
img_src), where save_path keeps the source file's name and so its extension (yolov6/core/inferer.py):
  * encode(frames, ...)     a list of uint8 [h, w, 3] BGR CUDA tensors (or one [B, h, w, 3]), optionally rectangles of them (jpeg_encode.crop_rects
                            gives save_one_box's) -> jpeg_encode.EncodedBatch: ONE pinned staging buffer, ONE host -> device copy, ten launches and
                            two memsets for the whole call whatever it holds (csrc/png_encode.hip), no host synchronisation;
  * EncodedBatch.files()    -> list[bytes]; the only call that synchronises.
What is written: 8-bit RGB (colour type 2), no interlace, ONE filter type for every row of a file ("sub" by default), and a zlib stream that
is exactly what zlib 1.2.11 gives for zlib.compressobj(1, zlib.DEFLATED, 15, 8, zlib.Z_RLE) over the filtered rows; it begins 78 01.  The file
around it is ours: the signature, IHDR, ONE IDAT chunk with the whole stream, IEND, correct CRC-32s, no ancillary chunks.  The rules are
restated in tests/png_encode_ref.py and pinned there to the interpreter's zlib module.

cv2.imwrite itself — UNCHECKED, OpenCV is not installed where this was written.  It drives libpng with PNG_FILTER_SUB on every row,
Z_BEST_SPEED (level 1), strategy Z_RLE, memLevel 8, window 15, and those are the settings pinned here; so the pixels and the deflate blocks
should be cv2's.  Byte identity of the FILE with cv2.imwrite is NOT claimed and nobody checks it: libpng rewrites the CMF byte of the zlib
header for small images (a smaller window) and splits the stream into IDAT chunks of 8192 bytes, where this module writes 78 01 and one chunk.
Parity is claimed with the zlib module only.  No CPU fallback.
The output buffer is sized from _worst_case_bytes.
Not done: gray, palette, alpha or 16-bit output; interlacing; other compression levels or strategies; adaptive (per-row) filter selection;
ancillary chunks (gAMA, pHYs, tEXt, ...).
"""
import ctypes as C

import numpy as np

from . import lib, png, staging
from .jpeg_encode import EncodedBatch
from .lib import MafError

FILTERS = {"none": 0, "sub": 1, "up": 2, "average": 3, "paeth": 4}
CHUNK = 4096                  # MAF_PNG_ENC_CHUNK
BLOCK_SYMBOLS = 16383         # MAF_PNG_ENC_BLOCK_SYMBOLS
CODE_WORDS = 320              # MAF_PNG_ENC_CODE_WORDS
HEAD_WORDS = 80               # MAF_PNG_ENC_HEAD_WORDS
FILE_BYTES = 57               # MAF_PNG_ENC_FILE_BYTES: signature 8, IHDR 25, IDAT length + type + CRC 12, IEND 12
STORED, FIXED, DYNAMIC, UNUSED = 0, 1, 2, -1      # MAF_PNG_ENC_*
MAX_RAW = 2 ** 31             # filtered bytes of one file, exclusive

HEADER_DT = np.dtype([("n_files", "<i4"), ("n_chunks", "<i4"), ("n_blocks", "<i4"), ("reserved", "<i4"), ("jobs_off", "<i8"), ("total_bytes", "<i8"),
                      ("raw_bytes", "<i8"), ("packed_bytes", "<i8"), ("out_bytes", "<i8")])   # maf_png_enc_header_t
JOB_DT = np.dtype([("src", "<u8"), ("pitch", "<i8"), ("raw_off", "<i8"), ("packed_off", "<i8"), ("packed_bytes", "<i8"), ("w", "<i4"), ("h", "<i4"),
                   ("filter", "<i4"), ("n_raw", "<i4"), ("chunk0", "<i4"), ("n_chunks", "<i4"), ("block0", "<i4"), ("n_blocks", "<i4")])   # maf_png_enc_job_t
BLOCK_DT = np.dtype([("bitoff", "<i8"), ("pos", "<i4"), ("type", "<i4"), ("bits", "<i4"), ("head_bits", "<i4"), ("n_sym", "<i4"),
                     ("stored_len", "<i4")])   # maf_png_enc_block_t


def _worst_case_bytes(n_raw):
    """Bytes the zlib stream of `n_raw` filtered bytes can take (MAF_PNG_ENC_ZBOUND): n_raw + 6 * (n_raw // 16383 + 1) + 6.  deflate writes every
    block in the cheapest of its three forms, so no block costs more than its stored form: 3 header bits, up to 7 bits of padding, LEN and NLEN
    (4 bytes), then the bytes it covers — under 6 bytes beside them (a block that is not stored is SHORTER than stored_len + 4 bytes: that is the
    test that chose it).  A file has at most n_raw // 16383 + 1 blocks, because a block closes after 16383 symbols and a symbol covers at least one
    byte; the stream adds 2 bytes in front (78 01) and the Adler-32 behind.  A file is FILE_BYTES more."""
    return n_raw + 6 * (n_raw // BLOCK_SYMBOLS + 1) + 6


# the hand-written binding of include/mafyolo_png_encode.h (tests/test_png_encode_host.py compares the two)
PROTOTYPES = {
    "maf_png_encode_struct_sizes": (C.c_int32, [C.POINTER(C.c_int32)]),
    "maf_png_encode": (C.c_int32, [C.c_void_p] * 14),
}
_bound = False


def _bind(L):
    """Set restype and argtypes of the two entry points on the handle lib.load() returns; a library without them is an error."""
    global _bound
    for name, (res, args) in PROTOTYPES.items():
        if not hasattr(L, name):
            raise MafError("libmafyolo_hip.so lacks %s (csrc/png_encode.hip): rebuild (__graft_entry__.build())" % name)
        fn = getattr(L, name)
        fn.restype, fn.argtypes = res, args
    _bound = True
    return L


def _library():
    L = lib.load()
    if not _bound:
        _bind(L)
    return staging.checked_library("png_encode", (("maf_png_encode_struct_sizes", 3),), [HEADER_DT.itemsize, JOB_DT.itemsize, BLOCK_DT.itemsize],
                                   "maf_png_enc_* structs")


assert png.MAX_SIDE == 65535   # the side staging.frame_list refuses above
_FRAME_TEXT = {      # staging.frame_list in encode()'s words
    "batch": "png_encode.encode: a tensor of frames is [B, h, w, 3], got %(shape)s",
    "none": "png_encode.encode: no frames",
    "not_tensor": "png_encode.encode: frame %(i)d is a %(kind)s, not a CUDA tensor",
    "cpu": "png_encode.encode runs on the HIP path only (no CPU fallback): frame %(i)d is on %(device)s",
    "device": "png_encode.encode: frame %(i)d is on %(device)s, frame 0 on %(first)s",
    "type": "png_encode.encode: frame %(i)d must be uint8 [h, w, 3] BGR, got %(dtype)s %(shape)s",
    "empty": "png_encode.encode: frame %(i)d is empty (%(w)d x %(h)d): there is no PNG file of an empty image",
    "too_large": "png_encode.encode: frame %(i)d is %(w)d x %(h)d, a side is at most 65535 (png.MAX_SIDE)",
    "stride": "png_encode.encode: frame %(i)d must have pixel stride 3 and channel stride 1 (any row pitch of at least 3 * w), got strides %(strides)s"}
_FRAME_TEXT["pitch"] = _FRAME_TEXT["stride"]


def encode(frames, filter="sub", rects=None, stream=None, taps=None):
    """Encode frames (a list of uint8 [h, w, 3] BGR CUDA tensors of any sizes, or one [B, h, w, 3] tensor; pixel stride 3, channel stride 1, any row
    pitch: read in place) to PNG files on the device -> EncodedBatch.  `filter`: "none", "sub" (cv2.imwrite's), "up", "average" or "paeth", the one
    filter type of every row.  `rects`: a host int array [R, 5] of (frame index, x1, y1, x2, y2): one file per rectangle frame[y1:y2, x1:x2]
    (jpeg_encode.crop_rects gives save_one_box's) instead of one per frame.  `stream`: a torch.cuda.Stream to work on (default: the current
    one).  Every buffer is sized on the host from _worst_case_bytes, so nothing is read back here.  `taps`: a dict that receives the
    intermediate buffers (raw, tok, blocks, packed, sums, the job table, the header) — tests and the probe."""
    import torch
    if not isinstance(filter, str) or filter not in FILTERS:
        raise MafError("png_encode.encode: filter is \"none\", \"sub\", \"up\", \"average\" or \"paeth\", got %r (adaptive selection is not done)" % (filter,))
    frames = staging.frame_list(frames, _FRAME_TEXT)
    fi, x1, y1, x2, y2 = staging.rect_list(frames, rects, "png_encode.encode", "PNG")
    fw = np.array([f.shape[1] for f in frames], np.int64)
    n = len(fi)
    if n > staging.MAX_FILES:
        raise MafError("png_encode.encode takes up to 65535 files per call")
    w, h = x2 - x1, y2 - y1
    n_raw = h * (1 + 3 * w)
    if n_raw.max() >= MAX_RAW:
        k = int(n_raw.argmax())
        raise MafError("png_encode.encode: file %d (%d x %d) has %d filtered bytes, fewer than 2 GiB are taken" % (k, w[k], h[k], n_raw[k]))
    pitch = np.maximum(np.array([f.stride(0) for f in frames], np.int64), 3 * fw)[fi]      # a one-row frame may carry any stride 0: it is never used
    base = np.array([f.data_ptr() for f in frames], np.uint64)[fi]
    raw_size = staging.align(n_raw)
    packed_size = staging.align(_worst_case_bytes(n_raw))
    nc = -(-packed_size // CHUNK)
    nb = n_raw // BLOCK_SYMBOLS + 1
    jobs = np.zeros(n, JOB_DT)
    jobs["src"] = base + (y1 * pitch + 3 * x1).astype(np.uint64)
    jobs["pitch"], jobs["w"], jobs["h"], jobs["filter"], jobs["n_raw"] = pitch, w, h, FILTERS[filter], n_raw
    jobs["raw_off"], jobs["packed_off"], jobs["packed_bytes"] = np.cumsum(raw_size) - raw_size, np.cumsum(packed_size) - packed_size, packed_size
    jobs["chunk0"], jobs["n_chunks"] = np.cumsum(nc) - nc, nc
    jobs["block0"], jobs["n_blocks"] = np.cumsum(nb) - nb, nb
    raw_bytes, packed_bytes, chunk, block = int(raw_size.sum()), int(packed_size.sum()), int(nc.sum()), int(nb.sum())
    out_bytes = int((FILE_BYTES + _worst_case_bytes(n_raw)).sum())          # per file: the frame of the file + the worst case of its stream
    if chunk >= 1 << 30 or block >= 1 << 30:
        raise MafError("png_encode.encode: %d chunks in one call, fewer than 2^30 are taken (split the batch)" % chunk)
    sections = (("jobs_off", jobs),)
    hdr, off = staging.blob_layout(HEADER_DT, sections)
    hdr["n_files"], hdr["n_chunks"], hdr["n_blocks"], hdr["total_bytes"] = n, chunk, block, off
    hdr["raw_bytes"], hdr["packed_bytes"], hdr["out_bytes"] = raw_bytes, packed_bytes, out_bytes
    if off >= staging.MAX_BLOB:
        raise MafError("png_encode.encode: the job table of one call is limited to 2 GiB")
    L = _library()
    dev = frames[0].device
    if stream is not None:
        for f in frames:
            f.record_stream(stream)                                          # the allocator must not hand a dropped frame on while `stream` still reads it
    with staging.staged(off, dev, stream, zeros=True) as s:                  # zeros: the alignment gaps are defined bytes
        staging.write_blob(s.host, hdr, sections)
        blob = s.copy()
        raw = torch.empty(raw_bytes, dtype=torch.uint8, device=dev)
        tok = torch.empty(raw_bytes, dtype=torch.int16, device=dev)          # uint16 on the device: a symbol covers at least one byte
        chunks = torch.empty(5 * chunk, dtype=torch.int32, device=dev)
        sums = torch.empty(4 * n, dtype=torch.int64, device=dev)             # zeroed by the library on the stream
        blocks = torch.empty(block * BLOCK_DT.itemsize, dtype=torch.uint8, device=dev)
        codes = torch.empty(block * CODE_WORDS, dtype=torch.int32, device=dev)
        heads = torch.empty(block * HEAD_WORDS, dtype=torch.int32, device=dev)
        packed = torch.empty(packed_bytes, dtype=torch.uint8, device=dev)    # zeroed by the library on the stream
        out = torch.empty(out_bytes, dtype=torch.uint8, device=dev)          # the files are written back to back
        lengths = torch.empty(n, dtype=torch.int32, device=dev)
        offsets = torch.empty(n, dtype=torch.int64, device=dev)
        lib.check(L.maf_png_encode(s.host.ctypes.data, blob.data_ptr(), raw.data_ptr(), tok.data_ptr(), chunks.data_ptr(), sums.data_ptr(), blocks.data_ptr(),
                                   codes.data_ptr(), heads.data_ptr(), packed.data_ptr(), out.data_ptr(), lengths.data_ptr(), offsets.data_ptr(),
                                   s.stream.cuda_stream))
    if taps is not None:
        taps.update(raw=raw, tok=tok, blocks=blocks, packed=packed, sums=sums, chunks=chunks, jobs=jobs, header=hdr)
    return EncodedBatch(out, offsets, lengths, s.stream, (frames, s.pinned, blob, raw, tok, chunks, sums, blocks, codes, heads, packed))
