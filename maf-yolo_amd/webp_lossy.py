"""File bytes in, frames out, on the device: lossy WebP decoding that equals libwebp's samples, bit for bit.

The other half of the reference's webp entry of IMG_FORMATS (yolov6/data/datasets.py load_image, LoadData of yolov6/core/inferer.py), beside
webp.py: a lossy WebP still is ONE VP8 key frame (RFC 6386) — no inter prediction, integer arithmetic that the format prescribes — followed
by libwebp's integer YUV -> BGR tail (the fancy upsampler, 14-bit fixed point):
  * parse(data)       host only: walks the RIFF chunks of one file (webp.riff_chunks, the walk webp.parse uses) and reads the 10 uncompressed
                      bytes of the first `VP8 ` chunk -> WebpLossyInfo.  Everything behind those bytes (the bool-coded frame header, the
                      partition sizes, the modes, the tokens) belongs to the device.  WebpUnsupported names everything outside the supported
                      set, MafError a corrupt file;
  * supported(data)   True where decode() takes the file;
  * decode(files)     a list of bytes-like objects or paths -> a list of uint8 [h_i, w_i, 3] BGR CUDA tensors: ONE pinned staging buffer, ONE
                      host -> device copy, one chain of launches for the whole call (csrc/vp8_decode.hip: parse, reconstruct, loop filter,
                      convert), no host synchronisation unless check=True reads the status words.
Why the frames are cv2.imread's: cv2.imread(IMREAD_COLOR) asks libwebp for WebPDecodeBGR, and that equals
Image.open(f).convert("RGBA")[..., 2::-1] of a Pillow linked against libwebp, which is what the fixtures hold (tools/make_golden_webp_lossy.py;
the system's libwebp 1.2.2 and Pillow's 1.6.0 gave identical planes and pixels on every file tried).  Identity with cv2 itself is NOT checked
anywhere in this repository (cv2 is not a dependency of its tests); the argument above stands for it.
Alpha is dropped, as cv2.imread(IMREAD_COLOR) drops it: an ALPH chunk is skipped and never decoded.  ICCP, XMP and unknown chunks are skipped.
EXIF: as in webp.py, an orientation other than 1 is refused unless decode(..., ignore_orientation=True) asks for the stored pixels.
Refused (WebpUnsupported): animations, lossless files (webp.decode takes those), such an orientation, a frame or a file beyond the staging limits.
A malformed bit stream is found on the device and reported as a status bit; the frame of such a file is all zero.  No CPU fallback.
The two entry points live in include/mafyolo_vp8.h, outside the signature table of mafyolo_hip.h, so this module binds them itself (_bind).
"""
import ctypes as C
from collections import namedtuple
from functools import partial

import numpy as np

from . import lib, staging, webp
from .lib import MafError
from .staging import align as _align, file_bytes
from .webp import WebpUnsupported

WebpLossyInfo = namedtuple("WebpLossyInfo", "width height stream first_partition profile has_alpha orientation extended")
# stream: (first byte, one past the last byte) of the `VP8 ` payload behind its 10 header bytes; first_partition: its size from the frame tag;
# has_alpha: the file has an ALPH chunk (dropped); orientation: the EXIF tag or None; extended: the file has a VP8X chunk

MAX_SIDE = 16383              # MAF_VP8_MAX_SIDE: 14-bit size fields
STREAM_PAD = 64               # MAF_VP8_STREAM_PAD
META_WORDS, MB_RECORD, MB_COEFFS = 64, 32, 384      # MAF_VP8_META_WORDS, MAF_VP8_MB_RECORD, MAF_VP8_MB_COEFFS
STAGE_PARSE, STAGE_RECON, STAGE_FILTER, STAGE_CONVERT, STAGE_ALL = 1, 2, 4, 8, 15

STATUS_INPUT_EXHAUSTED, STATUS_BAD_PARTITIONS = 1, 2   # MAF_VP8_ST_*
_STATUS_TEXT = ((STATUS_INPUT_EXHAUSTED, "a partition that ends early"),
                (STATUS_BAD_PARTITIONS, "partition sizes that run past the chunk or leave the last partition empty"))


def parse(data):
    """Walk the RIFF chunks of one WebP file (bytes-like or a path) and read the 10 header bytes of its `VP8 ` chunk -> WebpLossyInfo."""
    d = file_bytes(data)
    n = len(d)
    image = canvas = orientation = None
    extended = alpha = False
    for cc, body, L, p in webp.riff_chunks(d):
        if cc in (b"ANIM", b"ANMF"):
            raise WebpUnsupported("webp_lossy: an animation (an %s chunk) is not supported" % cc.decode("latin-1"))
        if cc == b"VP8X":
            canvas = webp.vp8x_canvas(d, body, L, p)
            extended = True
        elif cc == b"VP8L" and image is None:
            raise WebpUnsupported("webp_lossy: a lossless file (a 'VP8L' chunk) is not supported here: webp.decode takes it")
        elif cc == b"VP8 " and image is None:
            image = (body, body + L)
        elif cc == b"ALPH":
            alpha = True                                     # dropped: never decoded
        elif cc == b"EXIF":
            orientation = webp.exif_orientation(d, body, L, orientation)
    if image is None:
        raise MafError("webp_lossy: no image chunk (VP8 )")
    s, e = image
    if e - s < 10:
        raise MafError("webp_lossy: the VP8 chunk is shorter than its 10 header bytes")
    tag = int.from_bytes(d[s:s + 3], "little")
    key, profile, show, first = not tag & 1, tag >> 1 & 7, tag >> 4 & 1, tag >> 5
    if not key:
        raise MafError("webp_lossy: the VP8 frame is not a key frame")
    if profile > 3:
        raise MafError("webp_lossy: VP8 profile %d (0 to 3 exist)" % profile)
    if not show:
        raise MafError("webp_lossy: the VP8 frame is marked invisible")
    if d[s + 3:s + 6] != b"\x9d\x01\x2a":
        raise MafError("webp_lossy: the VP8 frame lacks the start code 9d 01 2a")
    w, h = (int.from_bytes(d[s + 6:s + 8], "little") & 0x3fff, int.from_bytes(d[s + 8:s + 10], "little") & 0x3fff)   # the upper 2 bits: a scale hint, ignored
    if w == 0 or h == 0:
        raise MafError("webp_lossy: a frame of %d x %d" % (w, h))
    if first > e - s - 10:
        raise MafError("webp_lossy: the first partition (%d bytes) runs past the VP8 chunk" % first)
    if canvas is not None and canvas != (w, h):
        raise MafError("webp_lossy: the VP8X canvas %d x %d disagrees with the VP8 size %d x %d" % (canvas + (w, h)))
    if 3 * w * h >= staging.MAX_BLOB or n >= staging.MAX_BLOB:
        raise WebpUnsupported("webp_lossy: %d x %d (%d file bytes) is beyond the %d bytes of a frame or a file decode() takes" % (w, h, n, staging.MAX_BLOB - 1))
    return WebpLossyInfo(w, h, (s + 10, e), first, profile, alpha, orientation, extended)


def _parse_for_decode(ignore_orientation, data):
    info = parse(data)
    if info.orientation not in (None, 1) and not ignore_orientation:
        raise WebpUnsupported("webp_lossy: an EXIF orientation of %d is not supported (what cv2.imread does with it depends on its version); "
                              "ignore_orientation=True decodes the stored pixels" % info.orientation)
    return info


def supported(data, ignore_orientation=False):
    """True where decode() takes this file (ignore_orientation=True: where decode(..., ignore_orientation=True) does)."""
    try:
        _parse_for_decode(ignore_orientation, data)
        return True
    except MafError:
        return False


# ---------------------------------------------------------------- the blob (host side)

IMAGE_DT = np.dtype([("stream_begin", "<i8"), ("stream_end", "<i8"), ("scratch_off", "<i8"), ("scratch_bytes", "<i8"), ("planes_off", "<i8"),
                     ("out_off", "<i8"), ("w", "<i4"), ("h", "<i4"), ("first_part_bytes", "<i4"), ("reserved", "<i4")])   # maf_vp8_image_t
HEADER_DT = np.dtype([("n_images", "<i4"), ("reserved", "<i4"), ("images_off", "<i8"), ("stream_off", "<i8"), ("stream_bytes", "<i8"),
                      ("total_bytes", "<i8"), ("scratch_bytes", "<i8"), ("plane_bytes", "<i8"), ("out_bytes", "<i8")])   # maf_vp8_header_t


def macroblocks(w, h):
    """(columns, rows) of 16 x 16 macroblocks."""
    return (w + 15) >> 4, (h + 15) >> 4


def scratch_bytes(w, h):
    """Bytes of an image's scratch region (the layout of include/mafyolo_vp8.h): the frame record, the macroblock records, the coefficients."""
    mbw, mbh = macroblocks(w, h)
    return META_WORDS * 4 + mbw * mbh * (MB_RECORD + 2 * MB_COEFFS)


def plane_views(planes, image):
    """The Y, U, V planes of one image (a record of the image table) as views of a plane buffer (`recon` or `yuv` of the taps), padded to whole
    macroblocks: Y [16 mbh, 16 mbw], U and V [8 mbh, 8 mbw]."""
    mbw, mbh = macroblocks(int(image["w"]), int(image["h"]))
    n, o = mbw * mbh, int(image["planes_off"])
    return (planes[o:o + 256 * n].view(16 * mbh, 16 * mbw), planes[o + 256 * n:o + 320 * n].view(8 * mbh, 8 * mbw),
            planes[o + 320 * n:o + 384 * n].view(8 * mbh, 8 * mbw))


def build_blob(infos):
    """Everything the device needs for one call, in one byte array: header | image table | the `VP8 ` payloads of every image (behind their
    10 header bytes) + STREAM_PAD zeros.  -> (header record, image table)."""
    B = len(infos)
    images = np.zeros(B, IMAGE_DT)
    at = scr = pl = outb = 0
    for im, info in zip(images, infos):
        nbytes = info.stream[1] - info.stream[0]
        mbw, mbh = macroblocks(info.width, info.height)
        im["stream_begin"], im["stream_end"] = at, at + nbytes
        im["w"], im["h"], im["first_part_bytes"] = info.width, info.height, info.first_partition
        im["scratch_off"], im["planes_off"], im["out_off"] = scr, pl, outb
        im["scratch_bytes"] = scratch_bytes(info.width, info.height)
        at += nbytes
        scr += int(im["scratch_bytes"])
        pl += 384 * mbw * mbh
        outb += _align(3 * info.width * info.height)
    hdr, off = staging.blob_layout(HEADER_DT, (("images_off", images),))
    hdr["n_images"] = B
    hdr["stream_off"] = off
    hdr["stream_bytes"] = _align(at + STREAM_PAD)
    hdr["total_bytes"] = off + _align(at + STREAM_PAD)
    hdr["scratch_bytes"], hdr["plane_bytes"], hdr["out_bytes"] = scr, pl, outb
    if max(int(hdr["total_bytes"]), scr, pl, outb) >= staging.MAX_BLOB or B > staging.MAX_FILES:
        raise MafError("webp_lossy: decode() takes up to 65535 files and 2 GiB of file bytes, frames and coefficients per call")
    return hdr, images


def fill_blob(buf, hdr, images, datas, infos):
    """Write the sections of build_blob into `buf` (a uint8 array of hdr.total_bytes: the pinned staging buffer)."""
    staging.write_blob(buf, hdr, (("images_off", images),))
    q = int(hdr["stream_off"])
    for d, info in zip(datas, infos):
        s, e = info.stream
        buf[q:q + e - s] = np.frombuffer(d, np.uint8, e - s, s)
        q += e - s
    buf[q:] = 0                                              # at least STREAM_PAD zero bytes


# The C-ABI of include/mafyolo_vp8.h, declared here (the signature table of the library covers mafyolo_hip.h only).  name -> (restype, argtypes)
PROTOTYPES = {
    "maf_vp8_struct_sizes": (C.c_int32, [C.POINTER(C.c_int32)]),
    "maf_vp8_decode": (C.c_int32, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p]),
}
_bound = False


def _bind(L):
    """Set restype and argtypes of the two entry points on the handle lib.load() returns; a library without them is an error."""
    global _bound
    for name, (res, args) in PROTOTYPES.items():
        if not hasattr(L, name):
            raise MafError("libmafyolo_hip.so lacks %s (csrc/vp8_decode.hip): rebuild (__graft_entry__.build())" % name)
        fn = getattr(L, name)
        fn.restype, fn.argtypes = res, args
    _bound = True
    return L


def _library():
    L = lib.load()
    if not _bound:
        _bind(L)
    return staging.checked_library("webp_lossy", (("maf_vp8_struct_sizes", 2),), [HEADER_DT.itemsize, IMAGE_DT.itemsize], "maf_vp8_* structs")


status_text = partial(staging.status_text, _STATUS_TEXT)


def decode(files, device=None, stream=None, check=True, stages=STAGE_ALL, taps=None, ignore_orientation=False):
    """Decode a list of lossy WebP files (bytes-like objects or paths; mixed sizes welcome) on the device -> a list of uint8 [h_i, w_i, 3]
    BGR CUDA tensors (views of one allocation), libwebp's WebPDecodeBGR samples (alpha dropped); they go into letterbox / eval_batch /
    detect_frames / train_batch as they are.  With check=True (the default) the per-image status words are read once after the launches (the
    call's one synchronisation) and a fault raises MafError naming the file and its status bits; check=False returns (frames, status int32
    [B]) without synchronising.  A file with a non-zero status has an all-zero frame.  `stream`: a torch.cuda.Stream to work on (default: the
    current one).  `ignore_orientation`: take a file whose EXIF orientation is not 1 and return its stored pixels.
    `taps`: a dict that receives `yuv` (uint8: the loop-filtered planes of every image, padded to whole macroblocks; plane_views(taps["yuv"],
    taps["images"][i]) gives Y, U, V of image i), `recon` (the same planes before the loop filter), `scratch`, the image table `images`,
    `status` and `header` — tests and the probe.
    `stages`: for the probe and the tests only; a mask without STAGE_PARSE neither sets the status words nor fills the buffers the later
    stages read, so the frames and the status of such a call mean nothing; decode with STAGE_ALL."""
    def build(datas, infos):
        hdr, images = build_blob(infos)
        return hdr, images, lambda host: fill_blob(host, hdr, images, datas, infos)

    def launch(L, s, blob, hdr, out, status):
        import torch
        scratch = torch.empty(int(hdr["scratch_bytes"]), dtype=torch.uint8, device=s.dev)
        recon = torch.empty(int(hdr["plane_bytes"]), dtype=torch.uint8, device=s.dev)
        yuv = torch.empty(int(hdr["plane_bytes"]), dtype=torch.uint8, device=s.dev)
        lib.check(L.maf_vp8_decode(s.host.ctypes.data, blob.data_ptr(), scratch.data_ptr(), recon.data_ptr(), yuv.data_ptr(), out.data_ptr(),
                                   status.data_ptr(), int(stages), s.stream.cuda_stream))
        return dict(yuv=yuv, recon=recon, scratch=scratch)

    return staging.decode_files("webp_lossy.decode", files, partial(_parse_for_decode, ignore_orientation), build, _library, launch, _STATUS_TEXT, True,
                                device, stream, check, taps)
