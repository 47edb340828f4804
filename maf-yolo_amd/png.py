"""File bytes in, frames out, on the device: PNG decoding that equals what cv2.imread (IMREAD_COLOR) returns, bit for bit.

The stage in front of letterbox.py / augment.py that the reference runs on the host, one file at a time, through cv2.imread, for the png
entries of IMG_FORMATS (yolov6/data/datasets.py load_image, LoadData of yolov6/core/inferer.py):
  * parse(data)       host only: walks the chunks of one file -> PngInfo (size, bit depth, colour type, palette, the IDAT byte ranges, the
                      expected inflated size h * (1 + rowbytes), for an Adam7 file the sum over its passes).  The CRC-32 of every critical chunk is checked (zlib.crc32).
                      PngUnsupported names everything outside the supported set, MafError a corrupt file;
  * supported(data)   True where decode() takes the file (a caller routes the others to the host decoder);
  * decode(files)     a list of bytes-like objects or paths -> a list of uint8 [h_i, w_i, 3] BGR CUDA tensors: ONE pinned staging buffer, ONE
                      host -> device copy, one chain of launches for the whole call (csrc/png_decode.hip: inflate, unfilter, convert), no
                      host synchronisation unless check=True reads the status words.
PNG is lossless, so the samples of a file are the same for every conforming decoder; what is left is the conversion OpenCV asks libpng for:
    RGB 8                    channels reversed to BGR
    RGBA 8                   alpha dropped (png_set_strip_alpha: no compositing), then BGR
    gray 8, gray + alpha 8   gray replicated to three channels, alpha dropped
    gray 1 / 2 / 4           expanded to 8 bit by x 255 / x 85 / x 17 (png_set_expand_gray_1_2_4_to_8), replicated
    palette 1 / 2 / 4 / 8    PLTE lookup (png_set_palette_to_rgb), BGR; tRNS ignored
    any 16-bit type          the HIGH byte of every sample (png_set_strip_16), then as the 8-bit type
tRNS only makes an alpha that is then dropped, so it is ignored everywhere; gAMA, sRGB, iCCP, pHYs, text and every other ancillary chunk are
skipped (their CRC is not checked), eXIf among them: no PNG file is rotated.  The Adler-32 at the end of the zlib stream is not verified.
Opt-in, interlaced=True on parse / supported / decode: Adam7 files (interlace method 1), in any mix with plain ones, from the same three
launches: every pass is a filter chain of its own for the unfilter kernel, and the convert kernel gathers each pixel from its pass (rules
restated in tests/png_adam7_ref.py).  Without the flag nothing changes.  Refused (PngUnsupported): Adam7 interlacing without the flag, any
other interlace method, a compression or filter method other than 0, a zlib header with a preset dictionary or a method other than deflate, APNG (an
acTL chunk), an unknown critical chunk, a side above 65535 or 2 GiB of scanlines.  A palette index past PLTE is found on the device and
reported as a status bit.  No CPU fallback.
"""
import struct
import zlib
from collections import namedtuple
from functools import partial

import numpy as np

from . import lib, staging
from .lib import MafError
from .staging import align as _align, file_bytes


class PngUnsupported(MafError):
    """A well-formed PNG file outside the supported set (the message names the kind)."""


SIGNATURE = b"\x89PNG\r\n\x1a\n"
PngInfo = namedtuple("PngInfo", "width height bit_depth color_type palette idat inflated_size rowbytes channels bpp interlace", defaults=(0,))
# palette: uint8 [n, 3] RGB (colour type 3) or None; idat: ((first byte, one past the last byte), ...) of the IDAT payloads in file order (their
# concatenation is the zlib stream); inflated_size = height * (1 + rowbytes), for an Adam7 file the sum of ph * (1 + prb) over its non-empty
# passes; bpp: the filters' byte distance max(1, channels * bit_depth / 8); interlace: IHDR's interlace method, 0 or 1 (Adam7)

CHANNELS = {0: 1, 2: 3, 3: 1, 4: 2, 6: 4}
DEPTHS = {0: (1, 2, 4, 8, 16), 2: (8, 16), 3: (1, 2, 4, 8), 4: (8, 16), 6: (8, 16)}
MAX_SIDE = 65535              # the limit jpeg.py has from its 16-bit fields
ADAM7 = ((0, 0, 8, 8), (4, 0, 8, 8), (0, 4, 4, 8), (2, 0, 4, 4), (0, 2, 2, 4), (1, 0, 2, 2), (0, 1, 1, 2))    # per pass: x0, y0, dx, dy (PNG 1.2, 8.2)

(STATUS_INPUT_EXHAUSTED, STATUS_BAD_BLOCK_TYPE, STATUS_BAD_STORED_LEN, STATUS_BAD_CODE_LENGTHS, STATUS_NO_CODE, STATUS_DISTANCE_TOO_FAR,
 STATUS_TOO_MANY_BYTES, STATUS_TOO_FEW_BYTES, STATUS_BAD_FILTER, STATUS_BAD_PALETTE_INDEX) = (1 << i for i in range(10))   # MAF_PNG_ST_*
_STATUS_TEXT = ((STATUS_INPUT_EXHAUSTED, "a deflate stream that ends early"), (STATUS_BAD_BLOCK_TYPE, "an invalid deflate block type"),
                (STATUS_BAD_STORED_LEN, "a stored block whose length check fails"), (STATUS_BAD_CODE_LENGTHS, "an invalid set of code lengths"),
                (STATUS_NO_CODE, "bits that match no Huffman code"), (STATUS_DISTANCE_TOO_FAR, "a distance that reaches before the start of the output"),
                (STATUS_TOO_MANY_BYTES, "more scanline bytes than the image holds"), (STATUS_TOO_FEW_BYTES, "fewer scanline bytes than the image holds"),
                (STATUS_BAD_FILTER, "a filter type above 4"), (STATUS_BAD_PALETTE_INDEX, "a palette index past PLTE"))


def adam7_passes(w, h, bits):
    """The seven passes of a w x h Adam7 image with `bits` bits per pixel -> [(pw, ph, prb)]: pixels per row, rows, bytes per row of the
    pass's sub-image.  A pass with pw == 0 or ph == 0 is absent from the stream (no filter bytes either)."""
    out = []
    for x0, y0, dx, dy in ADAM7:
        pw, ph = max(0, -(-(w - x0) // dx)), max(0, -(-(h - y0) // dy))
        out.append((pw, ph, (pw * bits + 7) // 8))
    return out


def adam7_sizes(w, h, bits):
    """(the inflated size, the bytes of the unfiltered sub-images back to back) of an Adam7 image."""
    live = [(ph, prb) for pw, ph, prb in adam7_passes(w, h, bits) if pw and ph]
    return sum(ph * (1 + prb) for ph, prb in live), sum(ph * prb for ph, prb in live)


def rows_size(info):
    """Bytes of the unfiltered rows of a parsed file: h * rowbytes, or the Adam7 sub-images back to back (more than that below 8 bits)."""
    if info.interlace:
        return adam7_sizes(info.width, info.height, info.channels * info.bit_depth)[1]
    return info.height * info.rowbytes


def parse(data, interlaced=False):
    """Walk the chunks of one PNG file (bytes-like or a path) -> PngInfo.  Host only.  interlaced=True also takes Adam7 files (interlace method 1)."""
    d = file_bytes(data)
    n = len(d)
    if d[:8] != SIGNATURE:
        raise MafError("png: no PNG signature at the start (not a PNG file)")
    p = 8
    ihdr = palette = None
    idat = []
    idat_closed = False
    seen_iend = False
    while p < n:
        if p + 8 > n:
            raise MafError("png: a chunk header runs past the end of the file")
        L, = struct.unpack(">I", d[p:p + 4])
        typ = d[p + 4:p + 8]
        if L > 0x7FFFFFFF or p + 12 + L > n:
            raise MafError("png: chunk %r runs past the end of the file" % typ.decode("latin-1"))
        body = p + 8
        critical = not typ[0] & 0x20
        if ihdr is None and typ != b"IHDR":
            raise MafError("png: the first chunk is %r, not IHDR" % typ.decode("latin-1"))
        if critical and zlib.crc32(d[p + 4:body + L]) != struct.unpack(">I", d[body + L:body + L + 4])[0]:
            raise MafError("png: the CRC-32 of chunk %s fails" % typ.decode("latin-1"))
        if typ == b"IHDR":
            if ihdr is not None or L != 13:
                raise MafError("png: a second or malformed IHDR chunk")
            ihdr = struct.unpack(">IIBBBBB", d[body:body + 13])
        elif typ == b"PLTE":
            if palette is not None or idat or L == 0 or L % 3 or L > 768:
                raise MafError("png: a misplaced or malformed PLTE chunk")
            palette = np.frombuffer(d, np.uint8, L, body).reshape(-1, 3).copy()
        elif typ == b"IDAT":
            if idat_closed:
                raise MafError("png: the IDAT chunks are not consecutive")
            idat.append((body, body + L))
        elif typ == b"IEND":
            seen_iend = True
            break
        elif typ == b"acTL":
            raise PngUnsupported("png: APNG (an acTL chunk) is not supported")
        elif critical:
            raise PngUnsupported("png: the unknown critical chunk %r is not supported" % typ.decode("latin-1"))
        if idat and typ != b"IDAT":
            idat_closed = True
        p = body + L + 4
    if ihdr is None:
        raise MafError("png: no IHDR chunk")
    w, h, depth, ctype, comp, filt, lace = ihdr
    if ctype not in DEPTHS or depth not in DEPTHS[ctype]:
        raise MafError("png: colour type %d with bit depth %d is not a PNG combination" % (ctype, depth))
    if w == 0 or h == 0:
        raise MafError("png: zero width or height")
    if comp != 0 or filt != 0:
        raise PngUnsupported("png: compression method %d / filter method %d is not supported (0 / 0 only)" % (comp, filt))
    if lace != 0 and not (interlaced and lace == 1):
        raise PngUnsupported("png: Adam7 interlacing is not supported" if lace == 1 else "png: interlace method %d is not supported" % lace)
    if w > MAX_SIDE or h > MAX_SIDE:
        raise PngUnsupported("png: %d x %d is beyond the %d x %d limit" % (w, h, MAX_SIDE, MAX_SIDE))
    if not idat:
        raise MafError("png: no IDAT chunk")
    if not seen_iend:
        raise MafError("png: no IEND chunk")
    if ctype == 3 and palette is None:
        raise MafError("png: a palette image without a PLTE chunk")
    head = b""
    for s, e in idat:                                        # the two bytes may lie in different chunks
        head += d[s:min(e, s + 2 - len(head))]
        if len(head) == 2:
            break
    if len(head) < 2:
        raise MafError("png: the IDAT chunks hold no zlib header")
    cmf, flg = head[0], head[1]
    if cmf & 15 != 8:
        raise PngUnsupported("png: zlib compression method %d is not supported (deflate only)" % (cmf & 15))
    if flg & 0x20:
        raise PngUnsupported("png: a zlib stream with a preset dictionary is not supported")
    if cmf >> 4 > 7 or (cmf * 256 + flg) % 31:
        raise MafError("png: a corrupt zlib header")
    ch = CHANNELS[ctype]
    rowbytes = (w * ch * depth + 7) // 8
    size = adam7_sizes(w, h, ch * depth)[0] if lace else h * (1 + rowbytes)
    if size >= 2 ** 31:
        raise PngUnsupported("png: %d x %d at %d bits per pixel is beyond the 2 GiB of scanlines decode() takes" % (w, h, ch * depth))
    return PngInfo(w, h, depth, ctype, palette if ctype == 3 else None, tuple(idat), size, rowbytes, ch, max(1, ch * depth // 8), lace)


def supported(data, interlaced=False):
    """True where decode() takes this file (interlaced=True: where decode(..., interlaced=True) does)."""
    try:
        parse(data, interlaced)
        return True
    except MafError:
        return False


# ---------------------------------------------------------------- the blob (host side)

IMAGE_DT = np.dtype([("stream_begin", "<i8"), ("stream_end", "<i8"), ("inf_off", "<i8"), ("rows_off", "<i8"), ("out_off", "<i8"), ("w", "<i4"),
                     ("h", "<i4"), ("depth", "<i4"), ("ctype", "<i4"), ("rowbytes", "<i4"), ("bpp", "<i4"), ("inflated_size", "<i4"), ("pal", "<i4"),
                     ("pal_n", "<i4"), ("interlace", "<i4")])   # maf_png_image_t
HEADER_DT = np.dtype([("n_images", "<i4"), ("n_palette", "<i4"), ("images_off", "<i8"), ("palette_off", "<i8"), ("stream_off", "<i8"),
                      ("stream_bytes", "<i8"), ("total_bytes", "<i8"), ("inflated_bytes", "<i8"), ("rows_bytes", "<i8"), ("out_bytes", "<i8")])   # maf_png_header_t
STREAM_PAD = 64               # zero bytes the host appends to the streams (the bit reader's clamp lands in them)
STAGE_INFLATE, STAGE_UNFILTER, STAGE_CONVERT, STAGE_ALL = 1, 2, 4, 7


def build_blob(infos):
    """Everything the device needs for one call, in one byte array: header | image table | palettes (B, G, R, 0 per entry) | the zlib streams of
    every image (IDAT payloads concatenated, chunk framing removed) + STREAM_PAD zeros.  -> (header record, image table, palette entries)."""
    B = len(infos)
    images = np.zeros(B, IMAGE_DT)
    pals = []
    at = inf = rows = outb = npal = 0
    for im, info in zip(images, infos):
        zbytes = sum(e - s for s, e in info.idat)
        im["stream_begin"], im["stream_end"] = at + 2, at + zbytes         # behind the 2-byte zlib header
        im["inf_off"], im["rows_off"], im["out_off"] = inf, rows, outb
        im["w"], im["h"], im["depth"], im["ctype"] = info.width, info.height, info.bit_depth, info.color_type
        im["rowbytes"], im["bpp"], im["inflated_size"], im["interlace"] = info.rowbytes, info.bpp, info.inflated_size, info.interlace
        if info.palette is not None:
            e = np.zeros((len(info.palette), 4), np.uint8)
            e[:, :3] = info.palette[:, ::-1]
            pals.append(e)
            im["pal"], im["pal_n"] = npal, len(e)
            npal += len(e)
        at += zbytes
        inf += _align(info.inflated_size)
        rows += _align(rows_size(info))
        outb += _align(3 * info.width * info.height)
    palette = np.concatenate(pals) if pals else np.zeros((0, 4), np.uint8)
    hdr, off = staging.blob_layout(HEADER_DT, (("images_off", images), ("palette_off", palette)))
    hdr["n_images"], hdr["n_palette"] = B, npal
    hdr["stream_off"] = off
    hdr["stream_bytes"] = _align(at + STREAM_PAD)            # a multiple of 8: the bit reader loads aligned 8-byte words
    hdr["total_bytes"] = off + _align(at + STREAM_PAD)
    hdr["inflated_bytes"], hdr["rows_bytes"], hdr["out_bytes"] = inf, rows, outb
    if hdr["total_bytes"] >= staging.MAX_BLOB or B > staging.MAX_FILES:
        raise MafError("png: decode() takes up to 65535 files and 2 GiB of file bytes per call")
    return hdr, images, palette


def fill_blob(buf, hdr, images, palette, datas, infos):
    """Write the sections of build_blob into `buf` (a uint8 array of hdr.total_bytes: the pinned staging buffer)."""
    staging.write_blob(buf, hdr, (("images_off", images), ("palette_off", palette)))
    q = int(hdr["stream_off"])
    for d, info in zip(datas, infos):
        for s, e in info.idat:
            buf[q:q + e - s] = np.frombuffer(d, np.uint8, e - s, s)
            q += e - s
    buf[q:] = 0                                              # at least STREAM_PAD zero bytes


_library = partial(staging.checked_library, "png", (("maf_png_struct_sizes", 2),), [HEADER_DT.itemsize, IMAGE_DT.itemsize], "maf_png_* structs")
status_text = partial(staging.status_text, _STATUS_TEXT)


def decode(files, device=None, stream=None, check=True, stages=STAGE_ALL, taps=None, interlaced=False):
    """Decode a list of PNG files (bytes-like objects or paths; mixed sizes, colour types and bit depths welcome) on the device; with
    interlaced=True the list may also hold Adam7 files, in any mix with plain ones (the same three launches: the unfilter kernel undoes each
    pass as a filter chain of its own, the convert kernel gathers every pixel from its pass).
    -> a list of uint8 [h_i, w_i, 3] BGR CUDA tensors (views of one allocation), what cv2.imread returns for each file; they go into
    letterbox / eval_batch / detect_frames / train_batch as they are.  With check=True (the default) the per-image status words are read
    once after the launches (the call's one synchronisation) and a fault raises MafError naming the file and its status bits; check=False
    returns (frames, status int32 [B]) without synchronising.  `stream`: a torch.cuda.Stream to work on (default: the current one).
    `taps`: a dict that receives the intermediate buffers (the inflated scanlines, the unfiltered rows, the image table) — tests and the probe.
    `stages`: for the probe and the tests only.  A mask without STAGE_INFLATE neither clears the status words nor fills the buffers the later
    stages read (they are fresh allocations here), so the frames and the status of such a call mean nothing; decode with STAGE_ALL."""
    def build(datas, infos):
        hdr, images, palette = build_blob(infos)
        return hdr, images, lambda host: fill_blob(host, hdr, images, palette, datas, infos)

    def launch(L, s, blob, hdr, out, status):
        import torch
        inflated = torch.empty(int(hdr["inflated_bytes"]), dtype=torch.uint8, device=s.dev)
        rows = torch.empty(int(hdr["rows_bytes"]), dtype=torch.uint8, device=s.dev)
        lib.check(L.maf_png_decode(s.host.ctypes.data, blob.data_ptr(), inflated.data_ptr(), rows.data_ptr(), out.data_ptr(), status.data_ptr(),
                                   int(stages), s.stream.cuda_stream))
        return dict(inflated=inflated, rows=rows)

    return staging.decode_files("png.decode", files, partial(parse, interlaced=True) if interlaced else parse, build, _library, launch, _STATUS_TEXT, True, device, stream, check, taps)
