"""Frames in, file bytes out, on the device: lossless WebP (VP8L) files that libwebp and this project's webp.decode return to the pixels that went in.

The last step of the reference's tools/infer.py for a .webp source, which it runs on the host one picture at a time: cv2.imwrite(save_path,
img_src), where save_path keeps the source file's name and so its extension (yolov6/core/inferer.py); without parameters cv2 writes lossless WebP:
  * encode(frames, ...)     a list of uint8 [h, w, 3] BGR CUDA tensors (or one [B, h, w, 3]), optionally rectangles of them (jpeg_encode.crop_rects
                            gives save_one_box's) -> jpeg_encode.EncodedBatch: ONE pinned staging buffer, ONE host -> device copy, fifteen launches
                            and three memsets for the whole call whatever it holds (csrc/webp_encode.hip), no host synchronisation;
  * EncodedBatch.files()    -> list[bytes]; the only call that synchronises.
What is written (the "profile", restated rule by rule in tests/webp_encode_ref.py, whose bytes the device equals): RIFF / WEBP with ONE VP8L chunk,
no VP8X and no metadata; subtract-green, then the predictor transform with `predictor_bits` and per block the mode with the lowest sum of
min(v, 256 - v) over the residual bytes (ties: the lowest mode); copies at distance 1 only, from a closed-form run rule (copies of at most 4096
pixels); no colour cache, no entropy image; five Huffman codes per image from the token counts, built as zlib builds its trees (csrc/png_trees.h),
limited to 15 bits (the code-length code to 7), written as simple codes where one or two symbols below 256 are used; the predictor sub-image goes
through the same tokeniser, codes and emitter as the main image.

What is claimed: the files are legal VP8L and decode, through libwebp (Pillow) and through webp.decode, to exactly the frames; the bytes are the
rule book's.  cv2.imwrite's own bytes are UNCHECKED and NOT claimed: libwebp's encoder follows heuristics (method, quality, entropy-image search,
cache sizing) that no specification fixes.  No CPU fallback.
The output buffer is sized from _worst_case_bytes.
Lossy WebP (VP8) is written by webp_lossy_encode.py.  Not done: alpha output; byte parity with libwebp's encoder; the cross-colour transform, colour indexing, the colour cache,
entropy images (more than one code group), backward references other than runs; VP8X, ICC / EXIF / XMP chunks; animation.
"""
import ctypes as C

import numpy as np

from . import lib, staging, webp
from .jpeg_encode import EncodedBatch
from .lib import MafError

CHUNK = 1024                  # MAF_WEBP_ENC_CHUNK
COPY_CHUNK = 4096             # MAF_WEBP_ENC_COPY_CHUNK
CODES = 5                     # MAF_WEBP_ENC_CODES
CODE_WORDS = 280              # MAF_WEBP_ENC_CODE_WORDS
HEAD_WORDS = 64               # MAF_WEBP_ENC_HEAD_WORDS
FILE_BYTES = 20               # MAF_WEBP_ENC_FILE_BYTES: RIFF, size, WEBP, VP8L, size
LEAD_BITS, MAIN_BITS = 50, 3  # MAF_WEBP_ENC_LEAD_BITS, MAF_WEBP_ENC_MAIN_BITS
MAX_SIDE = webp.MAX_SIDE      # 16384: the format's 14 bits

HEADER_DT = np.dtype([("n_files", "<i4"), ("n_images", "<i4"), ("n_chunks", "<i4"), ("n_blocks", "<i4"), ("n_copy", "<i4"), ("reserved", "<i4"),
                      ("jobs_off", "<i8"), ("images_off", "<i8"), ("total_bytes", "<i8"), ("px_words", "<i8"), ("packed_bytes", "<i8"),
                      ("out_bytes", "<i8")])   # maf_webp_enc_header_t
JOB_DT = np.dtype([("src", "<u8"), ("pitch", "<i8"), ("packed_off", "<i8"), ("packed_bytes", "<i8"), ("w", "<i4"), ("h", "<i4"), ("bits", "<i4"),
                   ("bw", "<i4"), ("block0", "<i4"), ("n_blocks", "<i4"), ("copy0", "<i4"), ("n_copy", "<i4")])   # maf_webp_enc_job_t
IMAGE_DT = np.dtype([("px_off", "<i8"), ("n_px", "<i4"), ("file", "<i4"), ("chunk0", "<i4"), ("n_chunks", "<i4"), ("main", "<i4"),
                     ("alpha", "<i4")])   # maf_webp_enc_image_t


def _worst_case_bytes(n_px, n_blocks):
    """Bytes the VP8L payload of a file of `n_px` pixels and `n_blocks` predictor blocks can take (MAF_WEBP_ENC_BOUND):
    ceil((50 + 3 + 2 * 5 * 2048 + 45 * (n_px + n_blocks)) / 8).
      * 50 bits lead the file (signature, sizes, the two transforms' headers, the sub-image's cache bit), 3 lead the main image;
      * each of the two images describes five codes.  A normal code's description is 1 + 4 + at most 19 * 3 + 1 bits and one token per code
        length at the most; a token is a code of the code-length code, limited to 7 bits, and the tokens 16 / 17 / 18 add 2 / 3 / 7 bits but stand
        for 3 / 3 / 11 lengths at the least, so no length costs more than 7 bits: 63 + 7 * 280 = 2023 bits, below the 2048 of HEAD_WORDS words;
      * a token covers at least one pixel (of the main image, or of the sub-image), so there are at most n_px + n_blocks tokens.  A literal is
        a green, a red and a blue code of at most 15 bits each — the alpha code has ONE used symbol in either image (0, 255) and is read with zero
        bits — so 45 bits; a copy is a length code of at most 15 bits, at most 10 extra bits, and the distance code, which has one symbol too.
    The bound is per token, not per file: a Huffman code never spends more than 8 bits per symbol on average over 256 symbols, which would give
    24 bits per pixel, but the 15-bit repair (zlib's gen_bitlen) is a heuristic whose result has no such proof.  Holding to what can be proved
    costs 45 / 24 of that memory: 5.6 bytes per pixel in `packed` and again in the output buffer (106 MiB for 32 frames of 640 x 480)."""
    return (LEAD_BITS + MAIN_BITS + 2 * CODES * 32 * HEAD_WORDS + 45 * (n_px + n_blocks) + 7) // 8


# the hand-written binding of include/mafyolo_webp_encode.h (tests/test_webp_encode_host.py compares the two)
PROTOTYPES = {
    "maf_webp_encode_struct_sizes": (C.c_int32, [C.POINTER(C.c_int32)]),
    "maf_webp_encode": (C.c_int32, [C.c_void_p] * 18),
}
_bound = False


def _bind(L):
    """Set restype and argtypes of the two entry points on the handle lib.load() returns; a library without them is an error."""
    global _bound
    for name, (res, args) in PROTOTYPES.items():
        if not hasattr(L, name):
            raise MafError("libmafyolo_hip.so lacks %s (csrc/webp_encode.hip): rebuild (__graft_entry__.build())" % name)
        fn = getattr(L, name)
        fn.restype, fn.argtypes = res, args
    _bound = True
    return L


def _library():
    L = lib.load()
    if not _bound:
        _bind(L)
    return staging.checked_library("webp_encode", (("maf_webp_encode_struct_sizes", 3),), [HEADER_DT.itemsize, JOB_DT.itemsize, IMAGE_DT.itemsize],
                                   "maf_webp_enc_* structs")


_FRAME_TEXT = {      # staging.frame_list in encode()'s words
    "batch": "webp_encode.encode: a tensor of frames is [B, h, w, 3], got %(shape)s",
    "none": "webp_encode.encode: no frames",
    "not_tensor": "webp_encode.encode: frame %(i)d is a %(kind)s, not a CUDA tensor",
    "cpu": "webp_encode.encode runs on the HIP path only (no CPU fallback): frame %(i)d is on %(device)s",
    "device": "webp_encode.encode: frame %(i)d is on %(device)s, frame 0 on %(first)s",
    "type": "webp_encode.encode: frame %(i)d must be uint8 [h, w, 3] BGR, got %(dtype)s %(shape)s",
    "empty": "webp_encode.encode: frame %(i)d is empty (%(w)d x %(h)d): there is no WebP file of an empty image",
    "too_large": "webp_encode.encode: frame %(i)d is %(w)d x %(h)d, a side is at most 65535",
    "stride": "webp_encode.encode: frame %(i)d must have pixel stride 3 and channel stride 1 (any row pitch of at least 3 * w), got strides %(strides)s"}
_FRAME_TEXT["pitch"] = _FRAME_TEXT["stride"]


def encode(frames, predictor_bits=4, rects=None, stream=None, taps=None):
    """Encode frames (a list of uint8 [h, w, 3] BGR CUDA tensors of any sizes, or one [B, h, w, 3] tensor; pixel stride 3, channel stride 1, any row
    pitch: read in place) to lossless WebP files on the device -> EncodedBatch.  `predictor_bits`: 2 .. 9, the predictor transform's blocks are
    2^bits pixels square.  `rects`: a host int array [R, 5] of (frame index, x1, y1, x2, y2): one file per rectangle frame[y1:y2, x1:x2]
    (jpeg_encode.crop_rects gives save_one_box's) instead of one per frame; a file's side is at most 16384.  `stream`: a torch.cuda.Stream to
    work on (default: the current one).  Every buffer is sized on the host from _worst_case_bytes, so nothing is read back here.  `taps`: a
    dict that receives the intermediate buffers (argb, modes, px (the sub-images and the residuals), tok, hist, codes (lengths and codes), sums
    (token counts, bits, bit offsets), packed, the job and image tables, the header) — tests and the probe."""
    import torch
    if isinstance(predictor_bits, bool) or not isinstance(predictor_bits, (int, np.integer)) or not 2 <= predictor_bits <= 9:
        raise MafError("webp_encode.encode: predictor_bits is an int from 2 to 9, got %r" % (predictor_bits,))
    frames = staging.frame_list(frames, _FRAME_TEXT)
    fi, x1, y1, x2, y2 = staging.rect_list(frames, rects, "webp_encode.encode", "WebP")
    fw = np.array([f.shape[1] for f in frames], np.int64)
    n = len(fi)
    if n > staging.MAX_FILES:
        raise MafError("webp_encode.encode takes up to 65535 files per call")
    w, h = x2 - x1, y2 - y1
    side = np.maximum(w, h)
    if side.max() > MAX_SIDE:
        k = int(side.argmax())
        raise MafError("webp_encode.encode: file %d is %d x %d, a side is at most 16384 (webp.MAX_SIDE)" % (k, w[k], h[k]))
    bits = int(predictor_bits)
    pitch = np.maximum(np.array([f.stride(0) for f in frames], np.int64), 3 * fw)[fi]      # a one-row frame may carry any stride 0: it is never used
    base = np.array([f.data_ptr() for f in frames], np.uint64)[fi]
    bw, bh = (w + (1 << bits) - 1) >> bits, (h + (1 << bits) - 1) >> bits
    n_px, nb = w * h, bw * bh
    packed_size = staging.align(_worst_case_bytes(n_px, nb))
    ncopy = -(-packed_size // COPY_CHUNK)
    jobs = np.zeros(n, JOB_DT)
    jobs["src"] = base + (y1 * pitch + 3 * x1).astype(np.uint64)
    jobs["pitch"], jobs["w"], jobs["h"], jobs["bits"], jobs["bw"] = pitch, w, h, bits, bw
    jobs["packed_off"], jobs["packed_bytes"] = np.cumsum(packed_size) - packed_size, packed_size
    jobs["block0"], jobs["n_blocks"] = np.cumsum(nb) - nb, nb
    jobs["copy0"], jobs["n_copy"] = np.cumsum(ncopy) - ncopy, ncopy
    images = np.zeros(2 * n, IMAGE_DT)                                       # per file: its sub-image, then its residuals
    images["n_px"][0::2], images["n_px"][1::2] = nb, n_px
    images["file"] = np.repeat(np.arange(n), 2)
    images["main"][1::2], images["alpha"][0::2] = 1, 255
    words = staging.align(images["n_px"].astype(np.int64), 4)
    nc = -(-images["n_px"].astype(np.int64) // CHUNK)
    images["px_off"], images["chunk0"], images["n_chunks"] = np.cumsum(words) - words, np.cumsum(nc) - nc, nc
    px_words, packed_bytes, chunk, block, copy = int(words.sum()), int(packed_size.sum()), int(nc.sum()), int(nb.sum()), int(ncopy.sum())
    out_bytes = int((FILE_BYTES + _worst_case_bytes(n_px, nb) + 1).sum())    # per file: the frame of the file, the worst case of its payload, the pad byte
    if chunk >= 1 << 30 or block >= 1 << 30 or copy >= 1 << 30:
        raise MafError("webp_encode.encode: %d chunks in one call, fewer than 2^30 are taken (split the batch)" % max(chunk, copy))
    sections = (("jobs_off", jobs), ("images_off", images))
    hdr, off = staging.blob_layout(HEADER_DT, sections)
    hdr["n_files"], hdr["n_images"], hdr["n_chunks"], hdr["n_blocks"], hdr["n_copy"], hdr["total_bytes"] = n, 2 * n, chunk, block, copy, off
    hdr["px_words"], hdr["packed_bytes"], hdr["out_bytes"] = px_words, packed_bytes, out_bytes
    if off >= staging.MAX_BLOB:
        raise MafError("webp_encode.encode: the job table of one call is limited to 2 GiB")
    L = _library()
    dev = frames[0].device
    if stream is not None:
        for f in frames:
            f.record_stream(stream)                                          # the allocator must not hand a dropped frame on while `stream` still reads it
    with staging.staged(off, dev, stream, zeros=True) as s:                  # zeros: the alignment gaps are defined bytes
        staging.write_blob(s.host, hdr, sections)
        blob = s.copy()
        argb = torch.empty(px_words, dtype=torch.int32, device=dev)
        px = torch.empty(px_words, dtype=torch.int32, device=dev)
        tok = torch.empty(px_words, dtype=torch.int32, device=dev)           # a token covers at least one pixel
        modes = torch.empty(block, dtype=torch.int32, device=dev)
        chunks = torch.empty(6 * chunk, dtype=torch.int32, device=dev)
        cbits = torch.empty(chunk, dtype=torch.int64, device=dev)
        hist = torch.empty(2 * n * CODES * CODE_WORDS, dtype=torch.int32, device=dev)      # zeroed by the library on the stream
        sums = torch.empty(4 * 2 * n, dtype=torch.int64, device=dev)         # zeroed by the library on the stream
        cinfo = torch.empty(8 * 2 * n, dtype=torch.int32, device=dev)
        codes = torch.empty(2 * n * CODES * CODE_WORDS, dtype=torch.int32, device=dev)
        heads = torch.empty(2 * n * CODES * HEAD_WORDS, dtype=torch.int32, device=dev)
        packed = torch.empty(packed_bytes, dtype=torch.uint8, device=dev)    # zeroed by the library on the stream
        out = torch.empty(out_bytes, dtype=torch.uint8, device=dev)          # the files are written back to back
        lengths = torch.empty(n, dtype=torch.int32, device=dev)
        offsets = torch.empty(n, dtype=torch.int64, device=dev)
        lib.check(L.maf_webp_encode(s.host.ctypes.data, blob.data_ptr(), argb.data_ptr(), px.data_ptr(), tok.data_ptr(), modes.data_ptr(), chunks.data_ptr(),
                                    cbits.data_ptr(), hist.data_ptr(), sums.data_ptr(), cinfo.data_ptr(), codes.data_ptr(), heads.data_ptr(), packed.data_ptr(),
                                    out.data_ptr(), lengths.data_ptr(), offsets.data_ptr(), s.stream.cuda_stream))
    if taps is not None:
        taps.update(argb=argb, modes=modes, px=px, tok=tok, hist=hist, codes=codes, sums=sums, cinfo=cinfo, packed=packed, chunks=chunks, jobs=jobs,
                    images=images, header=hdr)
    return EncodedBatch(out, offsets, lengths, s.stream, (frames, s.pinned, blob, argb, px, tok, modes, chunks, cbits, hist, sums, cinfo, codes, heads, packed))
