"""File bytes in, frames out, on the device: lossless WebP decoding that equals libwebp's samples, bit for bit.

The stage in front of letterbox.py / augment.py that the reference runs on the host, one file at a time, through cv2.imread, for the webp
entry of IMG_FORMATS (yolov6/data/datasets.py load_image, LoadData of yolov6/core/inferer.py) — the lossless half of it, the VP8L bit stream:
  * parse(data)       host only: walks the RIFF chunks of one file and reads the 5-byte VP8L header -> WebpInfo (size, alpha hint, the byte
                      range of the bit stream behind the header, the EXIF orientation, whether the file has a VP8X chunk).  Everything behind
                      those 5 bytes is inside the bit stream and belongs to the device.  WebpUnsupported names everything outside the supported
                      set, MafError a corrupt file;
  * supported(data)   True where decode() takes the file (a caller routes the others to the host decoder);
  * decode(files)     a list of bytes-like objects or paths -> a list of uint8 [h_i, w_i, 3] BGR CUDA tensors: ONE pinned staging buffer, ONE
                      host -> device copy, one chain of launches for the whole call (csrc/webp_decode.hip: entropy, inverse transforms,
                      convert), no host synchronisation unless check=True reads the status words.
Why the frames are cv2.imread's: VP8L is lossless, so the ARGB samples of a file are the same for every conforming decoder;
cv2.imread(IMREAD_COLOR) calls libwebp's WebPDecodeBGRInto, which returns those samples with alpha dropped (no compositing), and so does
Image.open(f).convert("RGBA")[..., 2::-1] of a Pillow linked against libwebp, which is what the fixtures hold (tools/make_golden_webp.py).
Identity with cv2 itself is NOT checked anywhere in this repository (cv2 is not a dependency of its tests); the argument above stands for it.
EXIF: what cv2 does with the orientation tag of a WebP file depends on the OpenCV version, which cannot be checked here, so a file whose EXIF
chunk carries an orientation other than 1 is refused (WebpUnsupported) unless decode(..., ignore_orientation=True) asks for the stored pixels.
Refused (WebpUnsupported): lossy files (a `VP8 ` chunk, with or without ALPH), animations (the VP8X animation flag, ANIM / ANMF chunks), a VP8L
version other than 0, such an orientation, 3 * w * h or the file bytes beyond the staging limits.  ICCP, XMP and unknown chunks are skipped.
A malformed bit stream is found on the device and reported as a status bit; the frame of such a file is all zero.  No CPU fallback.
The two entry points live in include/mafyolo_webp.h, outside the signature table of mafyolo_hip.h, so this module binds them itself (_bind).
"""
import ctypes as C
import struct
from collections import namedtuple
from functools import partial

import numpy as np

from . import jpeg, lib, staging
from .lib import MafError
from .staging import align as _align, file_bytes


class WebpUnsupported(MafError):
    """A well-formed WebP file outside the supported set (the message names the kind)."""


WebpInfo = namedtuple("WebpInfo", "width height has_alpha_hint stream orientation extended")
# stream: (first byte, one past the last byte) of the VP8L bit stream behind its 5 header bytes; orientation: the EXIF tag or None;
# extended: the file has a VP8X chunk

MAX_SIDE = 16384              # MAF_WEBP_MAX_SIDE: 14-bit size fields
STREAM_PAD = 64               # MAF_WEBP_STREAM_PAD
STAGE_ENTROPY, STAGE_TRANSFORM, STAGE_CONVERT, STAGE_ALL = 1, 2, 4, 7

(STATUS_INPUT_EXHAUSTED, STATUS_BAD_TRANSFORM, STATUS_BAD_CACHE_BITS, STATUS_BAD_CODE_LENGTHS, STATUS_NO_CODE, STATUS_DISTANCE_TOO_FAR,
 STATUS_COPY_PAST_END, STATUS_TABLE_SPACE) = (1 << i for i in range(8))   # MAF_WEBP_ST_*
_STATUS_TEXT = ((STATUS_INPUT_EXHAUSTED, "a bit stream that ends early"), (STATUS_BAD_TRANSFORM, "a transform type that appears twice"),
                (STATUS_BAD_CACHE_BITS, "colour cache bits outside 1 to 11"), (STATUS_BAD_CODE_LENGTHS, "an invalid set of code lengths"),
                (STATUS_NO_CODE, "bits that match no prefix code"), (STATUS_DISTANCE_TOO_FAR, "a distance that reaches before the start of the image"),
                (STATUS_COPY_PAST_END, "a copy that runs past the last pixel"), (STATUS_TABLE_SPACE, "more prefix codes than the stream length allows for"))


def riff_chunks(d):
    """The chunks of a RIFF / WEBP file in file order: (fourcc, first byte of the body, length of the body, offset of the chunk header).
    MafError where the container is broken, raised when the walk gets there.  webp_lossy.parse walks with it too."""
    n = len(d)
    if n < 12 or d[:4] != b"RIFF" or d[8:12] != b"WEBP":
        raise MafError("webp: no RIFF / WEBP signature at the start (not a WebP file)")
    riff_end = 8 + struct.unpack("<I", d[4:8])[0]
    if riff_end > n:
        raise MafError("webp: the RIFF size runs past the end of the file")
    p = 12
    while p < riff_end:
        if p + 8 > riff_end:
            raise MafError("webp: a chunk header runs past the end of the file")
        cc = d[p:p + 4]
        L, = struct.unpack("<I", d[p + 4:p + 8])
        body = p + 8
        if body + L > riff_end:
            raise MafError("webp: chunk %r runs past the end of the file" % cc.decode("latin-1"))
        yield cc, body, L, p
        p = body + L + (L & 1)


def vp8x_canvas(d, body, L, p):
    """The canvas (w, h) of a VP8X chunk; a misplaced or malformed one is a MafError, the animation flag WebpUnsupported."""
    if L < 10 or p != 12:
        raise MafError("webp: a misplaced or malformed VP8X chunk")
    if d[body] & 0x02:
        raise WebpUnsupported("webp: an animation (the VP8X animation flag) is not supported")
    return int.from_bytes(d[body + 4:body + 7], "little") + 1, int.from_bytes(d[body + 7:body + 10], "little") + 1


def exif_orientation(d, body, L, before):
    """The orientation tag of an EXIF chunk, or `before` where it has none."""
    seg = d[body:body + L]
    o = jpeg._exif_orientation(seg if seg[:6] == b"Exif\x00\x00" else b"Exif\x00\x00" + seg)
    return o if o is not None else before


def parse(data):
    """Walk the RIFF chunks of one WebP file (bytes-like or a path) and read the VP8L header -> WebpInfo.  Host only."""
    d = file_bytes(data)
    n = len(d)
    image = canvas = orientation = None
    extended = False
    for cc, body, L, p in riff_chunks(d):
        if cc == b"VP8 " or cc == b"ALPH":
            raise WebpUnsupported("webp: a lossy file (a %r chunk) is not supported (lossless VP8L only)" % cc.decode("latin-1"))
        if cc in (b"ANIM", b"ANMF"):
            raise WebpUnsupported("webp: an animation (an %s chunk) is not supported" % cc.decode("latin-1"))
        if cc == b"VP8X":
            canvas = vp8x_canvas(d, body, L, p)
            extended = True
        elif cc == b"VP8L" and image is None:
            image = (body, body + L)
        elif cc == b"EXIF":
            orientation = exif_orientation(d, body, L, orientation)
    if image is None:
        raise MafError("webp: no image chunk (VP8L)")
    s, e = image
    if e - s < 5 or d[s] != 0x2f:
        raise MafError("webp: the VP8L chunk does not start with the signature byte 0x2f")
    v = int.from_bytes(d[s + 1:s + 5], "little")
    w, h, alpha, version = (v & 0x3fff) + 1, (v >> 14 & 0x3fff) + 1, v >> 28 & 1, v >> 29
    if version != 0:
        raise WebpUnsupported("webp: VP8L version %d is not supported (0 only)" % version)
    if canvas is not None and canvas != (w, h):
        raise MafError("webp: the VP8X canvas %d x %d disagrees with the VP8L size %d x %d" % (canvas + (w, h)))
    if 3 * w * h >= staging.MAX_BLOB or n >= staging.MAX_BLOB:
        raise WebpUnsupported("webp: %d x %d (%d file bytes) is beyond the %d bytes of a frame or a file decode() takes" % (w, h, n, staging.MAX_BLOB - 1))
    return WebpInfo(w, h, bool(alpha), (s + 5, e), orientation, extended)


def _parse_for_decode(ignore_orientation, data):
    info = parse(data)
    if info.orientation not in (None, 1) and not ignore_orientation:
        raise WebpUnsupported("webp: an EXIF orientation of %d is not supported (what cv2.imread does with it depends on its version); "
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

IMAGE_DT = np.dtype([("stream_begin", "<i8"), ("stream_end", "<i8"), ("argb_off", "<i8"), ("scratch_off", "<i8"), ("scratch_bytes", "<i8"),
                     ("out_off", "<i8"), ("w", "<i4"), ("h", "<i4"), ("dir_words", "<i4"), ("arena_units", "<i4")])   # maf_webp_image_t
HEADER_DT = np.dtype([("n_images", "<i4"), ("reserved", "<i4"), ("images_off", "<i8"), ("stream_off", "<i8"), ("stream_bytes", "<i8"),
                      ("total_bytes", "<i8"), ("argb_words", "<i8"), ("scratch_bytes", "<i8"), ("out_bytes", "<i8")])   # maf_webp_header_t


def table_space(stream_bytes):
    """(dir_words, arena_units) of a stream of that many bytes: MAF_WEBP_DIR_WORDS / MAF_WEBP_ARENA_UNITS (the bound is derived in
    include/mafyolo_webp.h: a code costs at least 4 stream bits, a stored symbol at least a third of one)."""
    return 2 * stream_bytes + 40, 64 * stream_bytes + 64


def scratch_bytes(w, h, dir_words, arena_units):
    """Bytes of an image's scratch region (the layout of include/mafyolo_webp.h)."""
    sub = _align(-(-w // 4) * -(-h // 4) * 4)
    return 64 * 4 + 256 * 4 + 3 * sub + 2 * _align(w * h * 4) + _align(dir_words * 4) + _align(arena_units * 2)


def build_blob(infos):
    """Everything the device needs for one call, in one byte array: header | image table | the VP8L bit streams of every image (behind their
    5 header bytes) + STREAM_PAD zeros.  -> (header record, image table)."""
    B = len(infos)
    images = np.zeros(B, IMAGE_DT)
    at = argb = scr = outb = 0
    for im, info in zip(images, infos):
        nbytes = info.stream[1] - info.stream[0]
        im["stream_begin"], im["stream_end"] = at, at + nbytes
        im["w"], im["h"] = info.width, info.height
        im["dir_words"], im["arena_units"] = table_space(nbytes)
        im["argb_off"], im["scratch_off"], im["out_off"] = argb, scr, outb
        im["scratch_bytes"] = scratch_bytes(info.width, info.height, int(im["dir_words"]), int(im["arena_units"]))
        at += nbytes
        argb += _align(info.width * info.height, 4)
        scr += int(im["scratch_bytes"])
        outb += _align(3 * info.width * info.height)
    hdr, off = staging.blob_layout(HEADER_DT, (("images_off", images),))
    hdr["n_images"] = B
    hdr["stream_off"] = off
    hdr["stream_bytes"] = _align(at + STREAM_PAD)            # a multiple of 8: the bit reader loads aligned 8-byte words
    hdr["total_bytes"] = off + _align(at + STREAM_PAD)
    hdr["argb_words"], hdr["scratch_bytes"], hdr["out_bytes"] = argb, scr, outb
    if hdr["total_bytes"] >= staging.MAX_BLOB or B > staging.MAX_FILES:
        raise MafError("webp: decode() takes up to 65535 files and 2 GiB of file bytes per call")
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


# The C-ABI of include/mafyolo_webp.h, declared here (the signature table of the library covers mafyolo_hip.h only).  name -> (restype, argtypes)
PROTOTYPES = {
    "maf_webp_struct_sizes": (C.c_int32, [C.POINTER(C.c_int32)]),
    "maf_webp_decode": (C.c_int32, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p]),
}
_bound = False


def _bind(L):
    """Set restype and argtypes of the two entry points on the handle lib.load() returns; a library without them is an error."""
    global _bound
    for name, (res, args) in PROTOTYPES.items():
        if not hasattr(L, name):
            raise MafError("libmafyolo_hip.so lacks %s (csrc/webp_decode.hip): rebuild (__graft_entry__.build())" % name)
        fn = getattr(L, name)
        fn.restype, fn.argtypes = res, args
    _bound = True
    return L


def _library():
    L = lib.load()
    if not _bound:
        _bind(L)
    return staging.checked_library("webp", (("maf_webp_struct_sizes", 2),), [HEADER_DT.itemsize, IMAGE_DT.itemsize], "maf_webp_* structs")


status_text = partial(staging.status_text, _STATUS_TEXT)


def decode(files, device=None, stream=None, check=True, stages=STAGE_ALL, taps=None, ignore_orientation=False):
    """Decode a list of lossless WebP files (bytes-like objects or paths; mixed sizes welcome) on the device -> a list of uint8 [h_i, w_i, 3]
    BGR CUDA tensors (views of one allocation), libwebp's samples with alpha dropped; they go into letterbox / eval_batch / detect_frames /
    train_batch as they are.  With check=True (the default) the per-image status words are read once after the launches (the call's one
    synchronisation) and a fault raises MafError naming the file and its status bits; check=False returns (frames, status int32 [B]) without
    synchronising.  A file with a non-zero status has an all-zero frame.  `stream`: a torch.cuda.Stream to work on (default: the current one).
    `ignore_orientation`: take a file whose EXIF orientation is not 1 and return its stored pixels.
    `taps`: a dict that receives `argb` (uint32: per image, at images[i].argb_off, the main image after entropy decoding and before any
    inverse transform, h rows of the CODED width — narrower than w behind a palette of at most 16 colours; the later stages leave it as it is), `scratch`, the image table `images`, `status` and `header` — tests and the probe.
    `stages`: for the probe and the tests only; a mask without STAGE_ENTROPY neither clears the status words nor fills the buffers the later
    stages read, so the frames and the status of such a call mean nothing; decode with STAGE_ALL."""
    def build(datas, infos):
        hdr, images = build_blob(infos)
        return hdr, images, lambda host: fill_blob(host, hdr, images, datas, infos)

    def launch(L, s, blob, hdr, out, status):
        import torch
        argb = torch.empty(int(hdr["argb_words"]), dtype=torch.int32, device=s.dev)
        scratch = torch.empty(int(hdr["scratch_bytes"]), dtype=torch.uint8, device=s.dev)
        lib.check(L.maf_webp_decode(s.host.ctypes.data, blob.data_ptr(), argb.data_ptr(), scratch.data_ptr(), out.data_ptr(), status.data_ptr(),
                                    int(stages), s.stream.cuda_stream))
        return dict(argb=argb, scratch=scratch)

    return staging.decode_files("webp.decode", files, partial(_parse_for_decode, ignore_orientation), build, _library, launch, _STATUS_TEXT, True,
                                device, stream, check, taps)
