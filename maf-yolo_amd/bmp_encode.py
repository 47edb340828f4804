"""Frames in, file bytes out, on the device: BMP encoding, 24 bits, BI_RGB, bottom-up.

The last step of the reference's tools/infer.py for a .bmp source, which it runs on the host one picture at a time: cv2.imwrite(save_path,
img_src), where save_path keeps the source file's name and so its extension (yolov6/core/inferer.py):
  * encode(frames, ...)     a list of uint8 [h, w, 3] BGR CUDA tensors (or one [B, h, w, 3]), optionally rectangles of them (jpeg_encode.crop_rects
                            gives save_one_box's) -> jpeg_encode.EncodedBatch: ONE pinned staging buffer, ONE host -> device copy, ONE launch
                            for the whole call whatever it holds (csrc/bmp_encode.hip), no host synchronisation;
  * EncodedBatch.files()    -> list[bytes]; the only call that synchronises.
What is written: the 14-byte file header, a 40-byte BITMAPINFOHEADER, then the rows from the bottom one up, B, G, R per pixel as the frame
holds them, each row padded with zeros to a multiple of 4 bytes.  A file's size follows from its width and height, so the host places the
files and no scan runs on the device.  The layout is restated in tests/bmp_encode_ref.py; the pixel array is pinned to Pillow's.

cv2.imwrite itself — UNCHECKED, OpenCV is not installed where this was written.  As remembered, its writer fills in the file size and the
pixel offset 54, planes 1, bit count 24, compression 0 and leaves the five remaining DWORDs of the header 0, the image size included; that
is what is written here.  Byte identity of the FILE with cv2.imwrite is NOT claimed and nobody checks it.  No CPU fallback.
Not done: gray, palette, alpha, 16- or 32-bit output; RLE; top-down files; the V4 / V5 headers; resolution fields.
"""
import ctypes as C

import numpy as np

from . import lib, staging
from .jpeg_encode import EncodedBatch
from .lib import MafError

CHUNK = 4096                  # MAF_BMP_ENC_CHUNK
HEAD_BYTES = 54               # MAF_BMP_ENC_HEAD_BYTES
MAX_FILE = 1 << 31            # MAF_BMP_ENC_MAX_FILE: bytes of one file, exclusive

HEADER_DT = np.dtype([("n_files", "<i4"), ("n_chunks", "<i4"), ("jobs_off", "<i8"), ("total_bytes", "<i8"), ("out_bytes", "<i8")])   # maf_bmp_enc_header_t
JOB_DT = np.dtype([("src", "<u8"), ("pitch", "<i8"), ("out_off", "<i8"), ("w", "<i4"), ("h", "<i4"), ("chunk0", "<i4"), ("n_chunks", "<i4")])   # maf_bmp_enc_job_t

# the hand-written binding of include/mafyolo_bmp_encode.h (tests/test_bmp_encode_host.py compares the two)
PROTOTYPES = {
    "maf_bmp_encode_struct_sizes": (C.c_int32, [C.POINTER(C.c_int32)]),
    "maf_bmp_encode": (C.c_int32, [C.c_void_p] * 6),
}
_bound = False


def _bind(L):
    """Set restype and argtypes of the two entry points on the handle lib.load() returns; a library without them is an error."""
    global _bound
    for name, (res, args) in PROTOTYPES.items():
        if not hasattr(L, name):
            raise MafError("libmafyolo_hip.so lacks %s (csrc/bmp_encode.hip): rebuild (__graft_entry__.build())" % name)
        fn = getattr(L, name)
        fn.restype, fn.argtypes = res, args
    _bound = True
    return L


def _library():
    L = lib.load()
    if not _bound:
        _bind(L)
    return staging.checked_library("bmp_encode", (("maf_bmp_encode_struct_sizes", 2),), [HEADER_DT.itemsize, JOB_DT.itemsize], "maf_bmp_enc_* structs")


def file_bytes(w, h):
    """Bytes of the file of a w x h image: the headers and h rows of 3 * w bytes padded to a multiple of 4."""
    return HEAD_BYTES + (3 * w + 3) // 4 * 4 * h


_FRAME_TEXT = {      # staging.frame_list in encode()'s words
    "batch": "bmp_encode.encode: a tensor of frames is [B, h, w, 3], got %(shape)s",
    "none": "bmp_encode.encode: no frames",
    "not_tensor": "bmp_encode.encode: frame %(i)d is a %(kind)s, not a CUDA tensor",
    "cpu": "bmp_encode.encode runs on the HIP path only (no CPU fallback): frame %(i)d is on %(device)s",
    "device": "bmp_encode.encode: frame %(i)d is on %(device)s, frame 0 on %(first)s",
    "type": "bmp_encode.encode: frame %(i)d must be uint8 [h, w, 3] BGR, got %(dtype)s %(shape)s",
    "empty": "bmp_encode.encode: frame %(i)d is empty (%(w)d x %(h)d): there is no BMP file of an empty image",
    "too_large": "bmp_encode.encode: frame %(i)d is %(w)d x %(h)d, a side is at most 65535",
    "stride": "bmp_encode.encode: frame %(i)d must have pixel stride 3 and channel stride 1 (any row pitch of at least 3 * w), got strides %(strides)s"}
_FRAME_TEXT["pitch"] = _FRAME_TEXT["stride"]


def encode(frames, rects=None, stream=None):
    """Encode frames (a list of uint8 [h, w, 3] BGR CUDA tensors of any sizes, or one [B, h, w, 3] tensor; pixel stride 3, channel stride 1, any row
    pitch: read in place) to BMP files on the device -> EncodedBatch.  `rects`: a host int array [R, 5] of (frame index, x1, y1, x2, y2): one
    file per rectangle frame[y1:y2, x1:x2] (jpeg_encode.crop_rects gives save_one_box's) instead of one per frame.  `stream`: a
    torch.cuda.Stream to work on (default: the current one).  Nothing is read back here."""
    import torch
    frames = staging.frame_list(frames, _FRAME_TEXT)
    fi, x1, y1, x2, y2 = staging.rect_list(frames, rects, "bmp_encode.encode", "BMP")
    fw = np.array([f.shape[1] for f in frames], np.int64)
    n = len(fi)
    if n > staging.MAX_FILES:
        raise MafError("bmp_encode.encode takes up to 65535 files per call")
    w, h = x2 - x1, y2 - y1
    size = file_bytes(w, h)
    if size.max() >= MAX_FILE:
        k = int(size.argmax())
        raise MafError("bmp_encode.encode: file %d (%d x %d) has %d bytes, fewer than 2 GiB are taken" % (k, w[k], h[k], size[k]))
    pitch = np.maximum(np.array([f.stride(0) for f in frames], np.int64), 3 * fw)[fi]      # a one-row frame may carry any stride 0: it is never used
    base = np.array([f.data_ptr() for f in frames], np.uint64)[fi]
    end = np.cumsum(size)
    start = end - size
    nc = -(-end // CHUNK) - start // CHUNK
    jobs = np.zeros(n, JOB_DT)
    jobs["src"] = base + (y1 * pitch + 3 * x1).astype(np.uint64)
    jobs["pitch"], jobs["w"], jobs["h"], jobs["out_off"] = pitch, w, h, start
    jobs["chunk0"], jobs["n_chunks"] = np.cumsum(nc) - nc, nc
    chunks, out_bytes = int(nc.sum()), staging.align(int(end[-1]))
    if chunks >= 1 << 30:
        raise MafError("bmp_encode.encode: %d chunks in one call, fewer than 2^30 are taken (split the batch)" % chunks)
    sections = (("jobs_off", jobs),)
    hdr, off = staging.blob_layout(HEADER_DT, sections)
    hdr["n_files"], hdr["n_chunks"], hdr["total_bytes"], hdr["out_bytes"] = n, chunks, off, out_bytes
    if off >= staging.MAX_BLOB:
        raise MafError("bmp_encode.encode: the job table of one call is limited to 2 GiB")
    L = _library()
    dev = frames[0].device
    if stream is not None:
        for f in frames:
            f.record_stream(stream)                                          # the allocator must not hand a dropped frame on while `stream` still reads it
    with staging.staged(off, dev, stream, zeros=True) as s:                  # zeros: the alignment gaps are defined bytes
        staging.write_blob(s.host, hdr, sections)
        blob = s.copy()
        out = torch.empty(out_bytes, dtype=torch.uint8, device=dev)          # the files are written back to back
        lengths = torch.empty(n, dtype=torch.int32, device=dev)
        offsets = torch.empty(n, dtype=torch.int64, device=dev)
        lib.check(L.maf_bmp_encode(s.host.ctypes.data, blob.data_ptr(), out.data_ptr(), lengths.data_ptr(), offsets.data_ptr(), s.stream.cuda_stream))
    return EncodedBatch(out, offsets, lengths, s.stream, (frames, s.pinned, blob))
