"""File bytes in, frames out, on the device: BMP decoding that equals what Pillow's BmpImagePlugin gives, bit for bit.

The stage in front of letterbox.py / augment.py that the reference runs on the host, one file at a time, through cv2.imread, for the bmp entry of
IMG_FORMATS (yolov6/data/datasets.py load_image, LoadData of yolov6/core/inferer.py):
  * parse(data)       host only: reads the file header, the DIB header and the palette of one file -> BmpInfo (size, bits, compression,
                      direction, palette, the byte range of the pixel data).  BmpUnsupported names everything outside the supported set,
                      MafError a corrupt file;
  * supported(data)   True where decode() takes the file (a caller routes the others to the host decoder);
  * decode(files)     a list of bytes-like objects or paths -> a list of uint8 [h_i, w_i, 3] BGR CUDA tensors: ONE pinned staging buffer, ONE
                      host -> device copy, at most two launches for the whole call whatever the mix (csrc/bmp_decode.hip: one wave per RLE
                      file, then the conversion of every file), no host synchronisation unless check=True reads the status words.
Taken: the `BM` signature with a DIB header of 12 (OS/2 v1: 16-bit unsigned sizes, 3-byte palette entries), 40, 52, 56, 64, 108 or 124 bytes;
one plane; sides of 1 to 65535; a negative height (top-down rows) on uncompressed data; BI_RGB at 1, 4, 8, 24 and 32 bits (the 4th byte of a
32-bit pixel is dropped); BI_RLE8 at 8 bits and BI_RLE4 at 4 bits, bottom-up; BI_BITFIELDS at 32 bits with the masks (0xFF0000, 0xFF00, 0xFF)
and an alpha mask of 0 or 0xFF000000 (the alpha is dropped).  Rows are padded to 4 bytes and stored bottom-up, 1 and 4-bit pixels are packed MSB
first.  A palette holds `colors` entries (0 means 1 << bits, fewer are allowed) of B, G, R, x; an index at or above `colors` is black; a gap
between the palette and the pixel data (bfOffBits) is honoured.
RLE follows the format's rule, with a position (x, y) in file rows: an encoded run (n, v) writes n pixels (RLE4: the two nibbles of v in turn);
0 0 ends the line (x = 0, y + 1: on an empty row it skips that row, a full row stays on its row until it comes); 0 1 ends the bitmap; 0 2 dx dy
moves right and up; 0 n (n >= 3) is an absolute run of n pixels whose payload (RLE4: ceil(n / 2) bytes) is padded to even.  Pixels nothing
writes are index 0.  The walk stops once the position is at or past the last pixel, so data behind that is not looked at.  Pillow 12.2 departs
from the rule in three places (it drops the last pixel of an odd RLE4 absolute run, ignores an end of line on an empty row, raises on an early
end of bitmap); there the rule is still judged by Pillow, on an equivalent rewrite of the file (tests/bmp_ref.py rewrite).
Refused (BmpUnsupported, the message names the kind): every 16-bit file (Pillow scales 5-bit channels by 255 / 31, OpenCV shifts them: the two
disagree); every other BITFIELDS layout; BI_JPEG, BI_PNG and other compressions; top-down RLE; `colors` above 1 << bits; other header sizes and
bit depths; more than one plane; RLE data at an odd bfOffBits (Pillow aligns absolute runs by file position); a bfOffBits inside the headers or
the palette (Pillow then guesses); a gray ramp palette (entry i = i, i, i; two entries: 0 and 255) that is not the full 8-bit one or the 1-bit
black / white pair (Pillow drops such a palette and then misreads the packed rows).  Truncated uncompressed data is a MafError, as Pillow raises
on it too (parse wants the padding of the last row as well, which Pillow forgives).  A malformed RLE stream is found on the device and reported as status bits (the data ends without an end of bitmap before the last
row is complete; a run crosses its row's end, and is clamped there; a delta leaves the image); what follows the fault is index 0.  No CPU
fallback.

cv2.imread itself — UNCHECKED, OpenCV is not installed where this was written; argued from the sources (modules/imgcodecs/src/grfmt_bmp.cpp).
BmpDecoder::readHeader takes header sizes >= 36 and 12, reads `clrused` palette entries into a zero-filled 256-entry table (so an index past
them is black, as above), takes BI_RGB at 1 / 4 / 8 / 24 / 32 bits, RLE4 / RLE8 and 32-bit BITFIELDS; a negative height flips the origin.
readData walks the rows bottom-up with a 4-byte-aligned step, unpacks 1 and 4 bits MSB first through the palette (FillColorRow1 / 4 / 8), copies
24-bit rows and drops the 4th byte of 32-bit ones for a 3-channel destination; its RLE loops keep a position in the current line, fill the rest
of a line with palette index 0 on an end-of-line code and move by whole lines, and handle a delta as x + dx, y + dy — the rule above — and read
ceil(n / 2) payload bytes for an odd RLE4 absolute run.  So for every kind decode() takes the pixels should be cv2.imread's.  The kinds where
the two readers are known to differ (16-bit files) are the ones routed to the host.
"""
import ctypes as C
import struct
from collections import namedtuple
from functools import partial

import numpy as np

from . import lib, staging
from .lib import MafError
from .staging import align as _align, file_bytes


class BmpUnsupported(MafError):
    """A well-formed BMP file outside the supported set (the message names the kind)."""


BmpInfo = namedtuple("BmpInfo", "width height bits compression top_down header_size colors palette data row_bytes")
# compression: the header's value (0 BI_RGB, 1 BI_RLE8, 2 BI_RLE4, 3 BI_BITFIELDS); colors: the palette's entries (0 at 24 / 32 bits);
# palette: uint8 [colors, 3] in B, G, R order, or None; data: (first byte, one past the last byte) of the pixel data in the file (RLE: to
# the end of the file); row_bytes: the 4-byte-padded row of uncompressed data (RLE: 0)

MAX_SIDE = 65535                            # MAF_BMP_MAX_SIDE
MAX_ROWS_BYTES = 2 ** 31 - 2 ** 20          # the rows of one file, as in tiff.py
HEADER_SIZES = (12, 40, 52, 56, 64, 108, 124)
BI_RGB, BI_RLE8, BI_RLE4, BI_BITFIELDS = 0, 1, 2, 3
_COMPRESSION_NAMES = {4: "BI_JPEG", 5: "BI_PNG", 6: "BI_ALPHABITFIELDS", 11: "BI_CMYK", 12: "BI_CMYKRLE8", 13: "BI_CMYKRLE4"}
RGB_MASKS = (0xFF0000, 0xFF00, 0xFF)
ALPHA_MASKS = (0, 0xFF000000)

STATUS_INPUT_EXHAUSTED, STATUS_RUN_PAST_ROW, STATUS_DELTA_PAST_IMAGE = 1, 2, 4      # MAF_BMP_ST_*
_STATUS_TEXT = ((STATUS_INPUT_EXHAUSTED, "RLE data that ends with no end of bitmap before the last row is complete"),
                (STATUS_RUN_PAST_ROW, "an RLE run that crosses the end of its row"), (STATUS_DELTA_PAST_IMAGE, "an RLE delta that leaves the image"))


def _gray_ramp(entries, colors):
    """Pillow's test for a palette it drops: entry i is (i, i, i), or with two entries (0, 0, 0) and (255, 255, 255)."""
    ramp = np.array([0, 255] if colors == 2 else np.arange(colors) & 255, np.uint8)
    return bool((entries == ramp[:, None]).all())


def parse(data):
    """Read the headers and the palette of one BMP file (bytes-like or a path) -> BmpInfo.  Host only."""
    d = file_bytes(data)
    n = len(d)
    if d[:2] != b"BM":
        raise MafError("bmp: no BM signature at the start (not a BMP file)")
    if n < 18:
        raise MafError("bmp: the file header runs past the end of the file")
    off, hs = struct.unpack("<I", d[10:14])[0], struct.unpack("<I", d[14:18])[0]
    if hs not in HEADER_SIZES:
        raise BmpUnsupported("bmp: a DIB header of %d bytes is not supported (12, 40, 52, 56, 64, 108 or 124)" % hs)
    if 14 + hs > n:
        raise MafError("bmp: the DIB header (%d bytes) runs past the end of the file" % hs)
    if hs == 12:
        w, h, planes, bits = struct.unpack("<HHHH", d[18:26])
        compression, colors, entry = BI_RGB, 0, 3
    else:
        w, h, planes, bits, compression = struct.unpack("<iiHHI", d[18:34])
        colors, = struct.unpack("<I", d[46:50])
        entry = 4
    if w <= 0 or h == 0:
        raise MafError("bmp: zero or negative width, or zero height (%d x %d)" % (w, h))
    top_down, h = h < 0, abs(h)
    if planes != 1:
        raise BmpUnsupported("bmp: %d planes are not supported (1 only)" % planes)
    if bits == 16:
        raise BmpUnsupported("bmp: 16-bit files are not supported: the decoders disagree about them")
    if bits not in (1, 4, 8, 24, 32):
        raise BmpUnsupported("bmp: %d bits per pixel are not supported (1, 4, 8, 24 and 32 only)" % bits)
    head_end = 14 + hs
    if compression == BI_BITFIELDS and hs != 64:
        if hs == 40:
            head_end += 12                                       # the three masks follow the header
            if head_end > n:
                raise MafError("bmp: the BITFIELDS masks run past the end of the file")
        masks = struct.unpack("<III", d[54:66])
        alpha = struct.unpack("<I", d[66:70])[0] if hs >= 56 else 0
        if bits != 32 or masks != RGB_MASKS or alpha not in ALPHA_MASKS:
            raise BmpUnsupported("bmp: a BITFIELDS layout of %d bits with the masks %s and alpha 0x%x is not supported (32 bits, 0xff0000 0xff00 0xff, "
                                 "alpha 0 or 0xff000000 only)" % (bits, " ".join("0x%x" % m for m in masks), alpha))
    elif compression == BI_RLE8:
        if bits != 8:
            raise BmpUnsupported("bmp: compression BI_RLE8 at %d bits is not supported (8 bits only)" % bits)
    elif compression == BI_RLE4:
        if bits != 4:
            raise BmpUnsupported("bmp: compression BI_RLE4 at %d bits is not supported (4 bits only)" % bits)
    elif compression != BI_RGB:
        raise BmpUnsupported("bmp: compression %d%s is not supported (BI_RGB, BI_RLE8, BI_RLE4 and 32-bit BI_BITFIELDS only)" % (
            compression, " (%s)" % _COMPRESSION_NAMES[compression] if compression in _COMPRESSION_NAMES and hs != 64 else ""))
    rle = compression in (BI_RLE8, BI_RLE4)
    if rle and top_down:
        raise BmpUnsupported("bmp: top-down RLE (a negative height with BI_RLE%d) is not supported" % bits)
    if w > MAX_SIDE or h > MAX_SIDE:
        raise BmpUnsupported("bmp: %d x %d is beyond the %d x %d limit" % (w, h, MAX_SIDE, MAX_SIDE))
    row_bytes = (w * bits + 31) // 32 * 4
    if h * row_bytes >= MAX_ROWS_BYTES or 3 * w * h >= 2 ** 31:
        raise BmpUnsupported("bmp: %d x %d at %d bits per pixel is beyond the 2 GiB of rows decode() takes" % (w, h, bits))
    palette = None
    if bits <= 8:
        colors = colors or 1 << bits
        if colors > 1 << bits:
            raise BmpUnsupported("bmp: a palette of %d colors at %d bits is not supported (at most %d)" % (colors, bits, 1 << bits))
        if head_end + entry * colors > n:
            raise MafError("bmp: the palette (%d entries) runs past the end of the file" % colors)
        palette = np.frombuffer(d, np.uint8, entry * colors, head_end).reshape(colors, entry)[:, :3].copy()
        head_end += entry * colors
        if _gray_ramp(palette, colors) and (bits, colors) not in ((8, 256), (1, 2)):
            raise BmpUnsupported("bmp: a gray ramp palette of %d entries at %d bits is not supported: Pillow drops it and misreads the rows" % (colors, bits))
    else:
        colors = 0
    if off < head_end:
        raise BmpUnsupported("bmp: a pixel data offset (bfOffBits %d) inside the headers or the palette (%d bytes) is not supported" % (off, head_end))
    if off > n:
        raise MafError("bmp: the pixel data offset (bfOffBits %d) lies past the end of the file" % off)
    if rle:
        if off % 2:
            raise BmpUnsupported("bmp: RLE data at an odd offset (bfOffBits %d) is not supported: the decoders align absolute runs differently" % off)
        return BmpInfo(w, h, bits, compression, False, hs, colors, palette, (off, n), 0)
    if off + h * row_bytes > n:
        raise MafError("bmp: truncated pixel data (%d rows of %d bytes at offset %d in a file of %d bytes)" % (h, row_bytes, off, n))
    return BmpInfo(w, h, bits, compression, top_down, hs, colors, palette, (off, off + h * row_bytes), row_bytes)


def supported(data):
    """True where decode() takes this file."""
    try:
        parse(data)
        return True
    except MafError:
        return False


# ---------------------------------------------------------------- the blob (host side)

IMAGE_DT = np.dtype([("src_begin", "<i8"), ("src_end", "<i8"), ("plane_off", "<i8"), ("out_off", "<i8"), ("w", "<i4"), ("h", "<i4"), ("bits", "<i4"),
                     ("compression", "<i4"), ("row_bytes", "<i4"), ("top_down", "<i4"), ("pal", "<i4"), ("n_colors", "<i4")])   # maf_bmp_image_t
HEADER_DT = np.dtype([("n_images", "<i4"), ("n_rle", "<i4"), ("n_palette", "<i4"), ("reserved", "<i4"), ("images_off", "<i8"), ("rle_off", "<i8"),
                      ("palette_off", "<i8"), ("stream_off", "<i8"), ("stream_bytes", "<i8"), ("total_bytes", "<i8"), ("planes_bytes", "<i8"),
                      ("out_bytes", "<i8")])   # maf_bmp_header_t
STREAM_PAD = 64               # zero bytes the host appends to the pixel data (MAF_BMP_STREAM_PAD)


def build_blob(infos):
    """Everything the device needs for one call, in one byte array: header | image table | the RLE images' indices | palette entries (B, G, R, 0)
    | the pixel data of every file back to back (each on a 16-byte boundary) + STREAM_PAD zeros.
    -> (header record, image table, RLE list, palette entries)."""
    B = len(infos)
    images = np.zeros(B, IMAGE_DT)
    pals, rle = [], []
    at = planes = outb = npal = 0
    for k, (im, info) in enumerate(zip(images, infos)):
        nbytes = info.data[1] - info.data[0]
        im["src_begin"], im["src_end"], im["out_off"] = at, at + nbytes, outb
        im["w"], im["h"], im["bits"], im["row_bytes"], im["top_down"] = info.width, info.height, info.bits, info.row_bytes, int(info.top_down)
        im["compression"] = info.compression if info.compression in (BI_RLE8, BI_RLE4) else BI_RGB
        if info.compression in (BI_RLE8, BI_RLE4):
            rle.append(k)
            im["plane_off"] = planes
            planes += _align(info.width * info.height)
        if info.palette is not None:
            e = np.zeros((len(info.palette), 4), np.uint8)
            e[:, :3] = info.palette
            pals.append(e)
            im["pal"], im["n_colors"] = npal, len(e)
            npal += len(e)
        at = _align(at + nbytes)
        outb += _align(3 * info.width * info.height)
    palette = np.concatenate(pals) if pals else np.zeros((0, 4), np.uint8)
    rle = np.array(rle, "<i4")
    hdr, off = staging.blob_layout(HEADER_DT, (("images_off", images), ("rle_off", rle), ("palette_off", palette)))
    hdr["n_images"], hdr["n_rle"], hdr["n_palette"] = B, len(rle), npal
    hdr["stream_off"] = off
    hdr["stream_bytes"] = at + STREAM_PAD
    hdr["total_bytes"] = off + at + STREAM_PAD
    hdr["planes_bytes"], hdr["out_bytes"] = planes, outb
    if max(int(hdr["total_bytes"]), planes, outb) >= staging.MAX_BLOB or B > staging.MAX_FILES:
        raise MafError("bmp: decode() takes up to 65535 files and 2 GiB of file bytes, index planes and frames per call")
    return hdr, images, rle, palette


def fill_blob(buf, hdr, images, rle, palette, datas, infos):
    """Write the sections of build_blob into `buf` (a uint8 array of hdr.total_bytes: the pinned staging buffer)."""
    staging.write_blob(buf, hdr, (("images_off", images), ("rle_off", rle), ("palette_off", palette)))
    q = int(hdr["stream_off"])
    buf[q:] = 0                                                  # the gaps between the files and at least STREAM_PAD zero bytes behind them
    for d, im, info in zip(datas, images, infos):
        s, e = info.data
        buf[q + int(im["src_begin"]):q + int(im["src_end"])] = np.frombuffer(d, np.uint8, e - s, s)


# the hand-written binding of include/mafyolo_bmp.h (tests/test_bmp_host.py compares the two)
PROTOTYPES = {
    "maf_bmp_struct_sizes": (C.c_int32, [C.POINTER(C.c_int32)]),
    "maf_bmp_decode": (C.c_int32, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
}
_bound = False


def _bind(L):
    """Set restype and argtypes of the two entry points on the handle lib.load() returns; a library without them is an error."""
    global _bound
    for name, (res, args) in PROTOTYPES.items():
        if not hasattr(L, name):
            raise MafError("libmafyolo_hip.so lacks %s (csrc/bmp_decode.hip): rebuild (__graft_entry__.build())" % name)
        fn = getattr(L, name)
        fn.restype, fn.argtypes = res, args
    _bound = True
    return L


def _library():
    L = lib.load()
    if not _bound:
        _bind(L)
    return staging.checked_library("bmp", (("maf_bmp_struct_sizes", 2),), [HEADER_DT.itemsize, IMAGE_DT.itemsize], "maf_bmp_* structs")


status_text = partial(staging.status_text, _STATUS_TEXT)


def decode(files, device=None, stream=None, check=True, taps=None):
    """Decode a list of BMP files (bytes-like objects or paths; mixed sizes, bit depths, header kinds and compressions welcome) on the device
    -> a list of uint8 [h_i, w_i, 3] BGR CUDA tensors (views of one allocation), Pillow's pixels; they go into letterbox / eval_batch /
    detect_frames / train_batch as they are.  With check=True (the default) the per-image status words are read once after the launches (the
    call's one synchronisation) and a fault raises MafError naming the file and its status bits; check=False returns (frames, status int32
    [B]) without synchronising.  `stream`: a torch.cuda.Stream to work on (default: the current one).  `taps`: a dict that receives the
    intermediate buffers (the index planes of the RLE files, the image table and the RLE list) — tests and the probe."""
    tables = {}

    def build(datas, infos):
        hdr, images, rle, palette = build_blob(infos)
        tables["rle"] = rle
        return hdr, images, lambda host: fill_blob(host, hdr, images, rle, palette, datas, infos)

    def launch(L, s, blob, hdr, out, status):
        import torch
        planes = torch.empty(max(int(hdr["planes_bytes"]), 16), dtype=torch.uint8, device=s.dev)
        lib.check(L.maf_bmp_decode(s.host.ctypes.data, blob.data_ptr(), planes.data_ptr(), out.data_ptr(), status.data_ptr(), s.stream.cuda_stream))
        return dict(planes=planes, rle=tables["rle"])

    return staging.decode_files("bmp.decode", files, parse, build, _library, launch, _STATUS_TEXT, True, device, stream, check, taps)
