"""File bytes in, frames out, on the device: TIFF decoding that equals what libtiff gives Pillow, bit for bit.

The stage in front of letterbox.py / augment.py that the reference runs on the host, one file at a time, through cv2.imread, for the tif / tiff
entries of IMG_FORMATS (yolov6/data/datasets.py load_image, LoadData of yolov6/core/inferer.py):
  * parse(data)       host only: reads the header and the FIRST IFD of one file (the page cv2.imread and Pillow open) -> TiffInfo (size, bits,
                      samples, photometric, compression, predictor, the strips' byte ranges, the palette).  TiffUnsupported names everything
                      outside the supported set, MafError a corrupt file;
  * supported(data)   True where decode() takes the file (a caller routes the others to the host decoder);
  * decode(files)     a list of bytes-like objects or paths -> a list of uint8 [h_i, w_i, 3] BGR CUDA tensors: ONE pinned staging buffer, ONE
                      host -> device copy, two launches for the whole call whatever the mix (csrc/tiff_decode.hip: one wave per strip, then
                      predictor and conversion), no host synchronisation unless check=True reads the status words.
Taken: classic TIFF 6.0 in both byte orders; strips with any RowsPerStrip; PlanarConfiguration 1; FillOrder 1; Compression 1 (none), 5 (LZW),
32773 (PackBits), 8 and 32946 (Deflate, every strip a zlib stream of its own); Predictor 1, and 2 (horizontal differencing, 8-bit samples) on
LZW and Deflate.  The conversion, checked on the CPU against Pillow 12.2 / libtiff 4.7.1 (tests/tiff_ref.py restates the rules):
    Photometric 1 (BlackIsZero)   1 bit -> 0 / 255, 4 bit -> v * 17, 8 bit as it is; replicated to three channels
    Photometric 0 (WhiteIsZero)   the same, inverted (255 - x at 8 bits)
    Photometric 2 (RGB) 8 bit     three samples per pixel, written as BGR
    Photometric 3 (palette) 4 / 8 bit   ColorMap[v] >> 8 per channel
Rows are padded to whole bytes, samples below 8 bits are packed MSB first.
Refused (TiffUnsupported, the message names the kind): BigTIFF; tiles; PlanarConfiguration 2; 16 / 32-bit and float samples; 2-bit samples; any
ExtraSamples, or SamplesPerPixel other than 1 or 3 (libtiff's RGBA path premultiplies unassociated alpha, Pillow drops it: the two disagree);
Photometric other than 0 - 3; every other compression; FillOrder 2; an Orientation other than 1 unless ignore_orientation=True (Pillow applies
the tag on load); a palette whose entries are all below 256 (libtiff takes them as they are, Pillow shifts them to 0: no judge); a file with
a DNGVersion tag (its first IFD is a thumbnail); an LZW strip whose first 9 bits are not the Clear code 256 (the old LSB-first LZW too: libtiff
4.7.1 refuses such a strip).  A malformed strip is found on the device and reported as status bits; the rest of its rows is zero.  No CPU
fallback.

cv2.imread itself — UNCHECKED, OpenCV is not installed where this was written; argued from the sources.  For an 8-bit destination OpenCV's
TiffDecoder reads through libtiff's RGBA path (TIFFReadRGBAStrip), i.e. tif_getimage.c: gray maps through Map[x] = x * 255 / (2^bits - 1)
(x * 17 at 4 bits, 0 / 255 at 1 bit), MINISWHITE through (range - x) * 255 / range (255 - x at 8 bits), a palette through cvtcmap's
x >> 8 when any entry is above 255, RGB samples are copied; OpenCV then drops the (opaque) alpha and writes BGR.  Those are the rules above, and
the decompressors and the predictor are libtiff's own in both readers, so for every kind decode() takes the pixels should be cv2.imread's.  The
kinds where the RGBA path and Pillow differ (alpha, all-low palettes, orientation) are the ones routed to the host.
"""
import ctypes as C
import struct
from collections import namedtuple
from functools import partial

import numpy as np

from . import lib, staging
from .lib import MafError
from .staging import align as _align, file_bytes


class TiffUnsupported(MafError):
    """A well-formed TIFF file outside the supported set (the message names the kind)."""


TiffInfo = namedtuple("TiffInfo", "width height bits spp photometric compression predictor rows_per_strip strips palette row_bytes orientation byte_order")
# strips: ((first byte, one past the last byte), ...) of the ceil(height / rows_per_strip) strips in the file; rows_per_strip is clamped to
# height; palette: uint8 [1 << bits, 3] RGB (ColorMap >> 8) or None; compression: the tag's value (8 and 32946 both mean Deflate);
# byte_order: "<" or ">"

MAX_SIDE = 65535
MAX_STRIP_ROWS_BYTES = 2 ** 31 - 2 ** 20    # MAF_TIFF_MAX_STRIP_ROWS_BYTES: the rows of one strip, so of one image
COMP_NONE, COMP_LZW, COMP_DEFLATE, COMP_ADOBE_DEFLATE, COMP_PACKBITS = 1, 5, 32946, 8, 32773
COMPRESSIONS = (COMP_NONE, COMP_LZW, COMP_ADOBE_DEFLATE, COMP_DEFLATE, COMP_PACKBITS)
_TYPE_SIZE = {1: 1, 2: 1, 3: 2, 4: 4, 5: 8, 6: 1, 7: 1, 8: 2, 9: 4, 10: 8, 11: 4, 12: 8, 13: 4}
_INT_CODE = {1: "B", 3: "H", 4: "I", 6: "b", 8: "h", 9: "i", 13: "I"}
(T_WIDTH, T_HEIGHT, T_BITS, T_COMPRESSION, T_PHOTOMETRIC, T_FILL_ORDER, T_STRIP_OFFSETS, T_ORIENTATION, T_SPP, T_ROWS_PER_STRIP, T_STRIP_BYTES,
 T_PLANAR, T_PREDICTOR, T_COLORMAP, T_TILE_WIDTH, T_TILE_LENGTH, T_TILE_OFFSETS, T_TILE_BYTES, T_EXTRA_SAMPLES, T_SAMPLE_FORMAT, T_DNG_VERSION) = (
    256, 257, 258, 259, 262, 266, 273, 274, 277, 278, 279, 284, 317, 320, 322, 323, 324, 325, 338, 339, 50706)

STATUS_INPUT_EXHAUSTED, STATUS_LZW_BAD_CODE, STATUS_LZW_TABLE_FULL, STATUS_PACKBITS_OVERRUN = 1, 2, 4, 8      # MAF_TIFF_ST_*
STATUS_INFLATE_SHIFT = 8
_STATUS_TEXT = ((STATUS_INPUT_EXHAUSTED, "a strip that ends before its rows are full"), (STATUS_LZW_BAD_CODE, "an LZW code above the next free entry"),
                (STATUS_LZW_TABLE_FULL, "an LZW table pushed past 4095 entries"), (STATUS_PACKBITS_OVERRUN, "a PackBits literal or run that runs off its strip"),
                (0xBF << STATUS_INFLATE_SHIFT, "a corrupt Deflate strip"))


def ifd_entries(d):
    """The entries of the first IFD of a classic TIFF file -> (byte order "<" or ">", {tag: (type, count, where the values lie)}).  Raises
    MafError for anything that lies outside the file, TiffUnsupported for BigTIFF."""
    n = len(d)
    if d[:4] == b"II*\0":
        bo = "<"
    elif d[:4] == b"MM\0*":
        bo = ">"
    elif d[:4] in (b"II+\0", b"MM\0+"):
        raise TiffUnsupported("tiff: BigTIFF is not supported (classic TIFF only)")
    else:
        raise MafError("tiff: no TIFF signature at the start (not a TIFF file)")
    if n < 8:
        raise MafError("tiff: the header runs past the end of the file")
    at, = struct.unpack(bo + "I", d[4:8])
    if at < 8 or at + 2 > n:
        raise MafError("tiff: the offset of the first IFD (%d) lies past the end of the file" % at)
    count, = struct.unpack(bo + "H", d[at:at + 2])
    if at + 2 + 12 * count > n:
        raise MafError("tiff: the first IFD (%d entries) runs past the end of the file" % count)
    tags = {}
    for i in range(count):
        tag, typ, cnt, val = struct.unpack(bo + "HHII", d[at + 2 + 12 * i:at + 14 + 12 * i])
        size = _TYPE_SIZE.get(typ)
        if size is None:
            continue                                             # an unknown field type: skipped, as libtiff does
        if cnt * size > n:
            raise MafError("tiff: the count of tag %d (%d values of %d bytes) overflows the file" % (tag, cnt, size))
        where = at + 2 + 12 * i + 8 if cnt * size <= 4 else val
        if where + cnt * size > n:
            raise MafError("tiff: the values of tag %d lie at an offset past the end of the file" % tag)
        tags.setdefault(tag, (typ, cnt, where))
    return bo, tags


def _ints(d, bo, tags, tag, default=None):
    """The values of an integer tag as a list (default where the tag is absent)."""
    if tag not in tags:
        return default
    typ, cnt, where = tags[tag]
    if typ not in _INT_CODE:
        raise MafError("tiff: tag %d has field type %d, not an integer type" % (tag, typ))
    return list(struct.unpack(bo + "%d%s" % (cnt, _INT_CODE[typ]), d[where:where + cnt * _TYPE_SIZE[typ]]))


def parse(data, ignore_orientation=False):
    """Read the header and the first IFD of one TIFF file (bytes-like or a path) -> TiffInfo.  Host only.  ignore_orientation=True takes a
    file whose Orientation is not 1 (decode() then returns its stored pixels)."""
    d = file_bytes(data)
    bo, tags = ifd_entries(d)

    def one(tag, default):
        v = _ints(d, bo, tags, tag)
        if v is None:
            return default
        if not v:
            raise MafError("tiff: tag %d holds no value" % tag)
        return v[0]

    if T_DNG_VERSION in tags:
        raise TiffUnsupported("tiff: a DNG file (a DNGVersion tag) is not supported: its first IFD is a thumbnail")
    if any(t in tags for t in (T_TILE_WIDTH, T_TILE_LENGTH, T_TILE_OFFSETS, T_TILE_BYTES)):
        raise TiffUnsupported("tiff: tiles are not supported (strips only)")
    w, h = one(T_WIDTH, None), one(T_HEIGHT, None)
    if w is None or h is None:
        raise MafError("tiff: no ImageWidth or ImageLength tag")
    if w <= 0 or h <= 0:
        raise MafError("tiff: zero width or height")
    spp = one(T_SPP, 1)
    bits_all = _ints(d, bo, tags, T_BITS, [1])
    formats = _ints(d, bo, tags, T_SAMPLE_FORMAT, [1])
    if any(f != 1 for f in formats):
        raise TiffUnsupported("tiff: sample format %d (signed, float or undefined samples) is not supported (unsigned integers only)" % max(formats))
    if not bits_all or len(set(bits_all)) != 1:
        raise TiffUnsupported("tiff: samples of different bit depths %s are not supported" % bits_all)
    bits = bits_all[0]
    if bits in (16, 32, 64):
        raise TiffUnsupported("tiff: %d-bit samples are not supported (1, 4 and 8 bits only)" % bits)
    if bits == 2:
        raise TiffUnsupported("tiff: 2-bit samples are not supported (1, 4 and 8 bits only)")
    if bits not in (1, 4, 8):
        raise TiffUnsupported("tiff: %d-bit samples are not supported (1, 4 and 8 bits only)" % bits)
    if T_EXTRA_SAMPLES in tags and tags[T_EXTRA_SAMPLES][1] > 0:
        raise TiffUnsupported("tiff: ExtraSamples (an alpha or other extra channel) are not supported")
    if spp not in (1, 3):
        raise TiffUnsupported("tiff: %d samples per pixel are not supported (1 or 3 only)" % spp)
    if len(bits_all) not in (1, spp):
        raise MafError("tiff: BitsPerSample holds %d values for %d samples per pixel" % (len(bits_all), spp))
    photometric = one(T_PHOTOMETRIC, None)
    if photometric is None:
        raise TiffUnsupported("tiff: a file without a PhotometricInterpretation tag is not supported")
    if photometric not in (0, 1, 2, 3):
        raise TiffUnsupported("tiff: photometric interpretation %d is not supported (0 to 3 only)" % photometric)
    if (photometric == 2) != (spp == 3) or (photometric == 2 and bits != 8) or (photometric == 3 and bits == 1):
        raise TiffUnsupported("tiff: photometric interpretation %d with %d samples of %d bits is not supported" % (photometric, spp, bits))
    if one(T_PLANAR, 1) != 1 and spp > 1:
        raise TiffUnsupported("tiff: PlanarConfiguration 2 (separate planes) is not supported")
    compression = one(T_COMPRESSION, 1)
    if compression not in COMPRESSIONS:
        raise TiffUnsupported("tiff: compression %d is not supported (1 none, 5 LZW, 8 / 32946 Deflate, 32773 PackBits)" % compression)
    if one(T_FILL_ORDER, 1) != 1:
        raise TiffUnsupported("tiff: FillOrder 2 (least significant bit first) is not supported")
    orientation = one(T_ORIENTATION, 1)
    if orientation != 1 and not ignore_orientation:
        raise TiffUnsupported("tiff: an Orientation of %d is not supported (ignore_orientation=True returns the stored pixels)" % orientation)
    predictor = one(T_PREDICTOR, 1)
    if predictor not in (1, 2) or (predictor == 2 and (bits != 8 or compression in (COMP_NONE, COMP_PACKBITS))):
        raise TiffUnsupported("tiff: predictor %d with compression %d at %d bits is not supported (2 on LZW and Deflate at 8 bits only)" % (predictor, compression, bits))
    if w > MAX_SIDE or h > MAX_SIDE:
        raise TiffUnsupported("tiff: %d x %d is beyond the %d x %d limit" % (w, h, MAX_SIDE, MAX_SIDE))
    row_bytes = (w * spp * bits + 7) // 8
    if h * row_bytes >= MAX_STRIP_ROWS_BYTES or 3 * w * h >= 2 ** 31:
        raise TiffUnsupported("tiff: %d x %d at %d bits per pixel is beyond the 2 GiB of rows decode() takes" % (w, h, spp * bits))
    palette = None
    if photometric == 3:
        cmap = _ints(d, bo, tags, T_COLORMAP)
        if cmap is None or len(cmap) != 3 << bits or tags[T_COLORMAP][0] != 3:
            raise MafError("tiff: a palette image without a ColorMap of 3 x %d SHORT entries" % (1 << bits))
        if max(cmap) < 256:
            raise TiffUnsupported("tiff: a palette whose entries are all below 256 (an 8-bit ColorMap) is not supported: the decoders disagree about it")
        palette = (np.array(cmap, np.uint16).reshape(3, 1 << bits).T >> 8).astype(np.uint8)
    rps = min(max(one(T_ROWS_PER_STRIP, h), 0), h)
    if rps == 0:
        raise MafError("tiff: RowsPerStrip is 0")
    n_strips = -(-h // rps)
    offsets, counts = _ints(d, bo, tags, T_STRIP_OFFSETS), _ints(d, bo, tags, T_STRIP_BYTES)
    if offsets is None:
        raise MafError("tiff: no StripOffsets tag")
    if counts is None:
        raise TiffUnsupported("tiff: a file without a StripByteCounts tag is not supported")
    if len(offsets) < n_strips or len(counts) < n_strips:
        raise MafError("tiff: %d strip offsets and %d byte counts for the %d strips of %d rows at %d rows per strip" % (len(offsets), len(counts), n_strips, h, rps))
    strips = []
    for j in range(n_strips):
        s, c = offsets[j], counts[j]
        if s < 0 or c < 0 or s + c > len(d):
            raise MafError("tiff: strip %d (bytes %d to %d) lies outside the file of %d bytes" % (j, s, s + c, len(d)))
        if compression == COMP_LZW and (c < 2 or (d[s] << 1 | d[s + 1] >> 7) != 256):
            raise TiffUnsupported("tiff: an LZW strip that does not begin with the Clear code 256 (old-style LZW among them) is not supported")
        if compression in (COMP_DEFLATE, COMP_ADOBE_DEFLATE):
            if c < 2:
                raise MafError("tiff: Deflate strip %d holds no zlib header" % j)
            cmf, flg = d[s], d[s + 1]
            if cmf & 15 != 8:
                raise TiffUnsupported("tiff: zlib compression method %d is not supported (deflate only)" % (cmf & 15))
            if flg & 0x20:
                raise TiffUnsupported("tiff: a zlib stream with a preset dictionary is not supported")
            if cmf >> 4 > 7 or (cmf * 256 + flg) % 31:
                raise MafError("tiff: a corrupt zlib header in strip %d" % j)
        strips.append((s, s + c))
    return TiffInfo(w, h, bits, spp, photometric, compression, predictor, rps, tuple(strips), palette, row_bytes, orientation, bo)


def supported(data, ignore_orientation=False):
    """True where decode() takes this file (ignore_orientation=True: where decode(..., ignore_orientation=True) does)."""
    try:
        parse(data, ignore_orientation)
        return True
    except MafError:
        return False


# ---------------------------------------------------------------- the blob (host side)

IMAGE_DT = np.dtype([("rows_off", "<i8"), ("out_off", "<i8"), ("w", "<i4"), ("h", "<i4"), ("bits", "<i4"), ("spp", "<i4"), ("photometric", "<i4"),
                     ("predictor", "<i4"), ("row_bytes", "<i4"), ("pal", "<i4"), ("first_strip", "<i4"), ("n_strips", "<i4"), ("rows_per_strip", "<i4"),
                     ("reserved", "<i4")])   # maf_tiff_image_t
STRIP_DT = np.dtype([("src_begin", "<i8"), ("src_end", "<i8"), ("dst_off", "<i8"), ("dst_bytes", "<i4"), ("compression", "<i4"), ("image", "<i4"),
                     ("reserved", "<i4")])   # maf_tiff_strip_t
HEADER_DT = np.dtype([("n_images", "<i4"), ("n_strips", "<i4"), ("n_palette", "<i4"), ("reserved", "<i4"), ("images_off", "<i8"), ("strips_off", "<i8"),
                      ("palette_off", "<i8"), ("stream_off", "<i8"), ("stream_bytes", "<i8"), ("total_bytes", "<i8"), ("rows_bytes", "<i8"),
                      ("out_bytes", "<i8")])   # maf_tiff_header_t
STREAM_PAD = 64               # zero bytes the host appends to the strips (the inflate's clamp lands in them)
MAX_STRIPS = 1 << 24


def build_blob(infos):
    """Everything the device needs for one call, in one byte array: header | image table | strip table | palettes (B, G, R, 0 per entry) | the
    strips of every image back to back + STREAM_PAD zeros.  A Deflate strip travels without its 2-byte zlib header.
    -> (header record, image table, strip table, palette entries)."""
    B = len(infos)
    images = np.zeros(B, IMAGE_DT)
    strips = np.zeros(sum(len(i.strips) for i in infos), STRIP_DT)
    pals = []
    at = rows = outb = npal = ns = 0
    for k, (im, info) in enumerate(zip(images, infos)):
        im["rows_off"], im["out_off"] = rows, outb
        im["w"], im["h"], im["bits"], im["spp"] = info.width, info.height, info.bits, info.spp
        im["photometric"], im["predictor"], im["row_bytes"] = info.photometric, info.predictor, info.row_bytes
        im["first_strip"], im["n_strips"], im["rows_per_strip"] = ns, len(info.strips), info.rows_per_strip
        if info.palette is not None:
            e = np.zeros((len(info.palette), 4), np.uint8)
            e[:, :3] = info.palette[:, ::-1]
            pals.append(e)
            im["pal"] = npal
            npal += len(e)
        deflate = info.compression in (COMP_DEFLATE, COMP_ADOBE_DEFLATE)
        for j, (s, e) in enumerate(info.strips):
            sp = strips[ns + j]
            nbytes = e - s - (2 if deflate else 0)
            y0 = j * info.rows_per_strip
            sp["src_begin"], sp["src_end"] = at, at + nbytes
            sp["dst_off"] = rows + y0 * info.row_bytes
            sp["dst_bytes"] = min(info.rows_per_strip, info.height - y0) * info.row_bytes
            sp["compression"], sp["image"] = COMP_ADOBE_DEFLATE if deflate else info.compression, k
            at += nbytes
        ns += len(info.strips)
        rows += _align(info.height * info.row_bytes)
        outb += _align(3 * info.width * info.height)
    palette = np.concatenate(pals) if pals else np.zeros((0, 4), np.uint8)
    hdr, off = staging.blob_layout(HEADER_DT, (("images_off", images), ("strips_off", strips), ("palette_off", palette)))
    hdr["n_images"], hdr["n_strips"], hdr["n_palette"] = B, ns, npal
    hdr["stream_off"] = off
    hdr["stream_bytes"] = _align(at + STREAM_PAD)            # a multiple of 8: the inflate's bit reader loads aligned 8-byte words
    hdr["total_bytes"] = off + _align(at + STREAM_PAD)
    hdr["rows_bytes"], hdr["out_bytes"] = rows, outb
    if max(int(hdr["total_bytes"]), rows, outb) >= staging.MAX_BLOB or B > staging.MAX_FILES or ns > MAX_STRIPS:
        raise MafError("tiff: decode() takes up to 65535 files, %d strips and 2 GiB of file bytes, rows and frames per call" % MAX_STRIPS)
    return hdr, images, strips, palette


def fill_blob(buf, hdr, images, strips, palette, datas, infos):
    """Write the sections of build_blob into `buf` (a uint8 array of hdr.total_bytes: the pinned staging buffer)."""
    staging.write_blob(buf, hdr, (("images_off", images), ("strips_off", strips), ("palette_off", palette)))
    q = int(hdr["stream_off"])
    for d, info in zip(datas, infos):
        skip = 2 if info.compression in (COMP_DEFLATE, COMP_ADOBE_DEFLATE) else 0
        for s, e in info.strips:
            buf[q:q + e - s - skip] = np.frombuffer(d, np.uint8, e - s - skip, s + skip)
            q += e - s - skip
    buf[q:] = 0                                              # at least STREAM_PAD zero bytes


# the hand-written binding of include/mafyolo_tiff.h (tests/test_tiff_host.py compares the two)
PROTOTYPES = {
    "maf_tiff_struct_sizes": (C.c_int32, [C.POINTER(C.c_int32)]),
    "maf_tiff_decode": (C.c_int32, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
}
_bound = False


def _bind(L):
    """Set restype and argtypes of the two entry points on the handle lib.load() returns; a library without them is an error."""
    global _bound
    for name, (res, args) in PROTOTYPES.items():
        if not hasattr(L, name):
            raise MafError("libmafyolo_hip.so lacks %s (csrc/tiff_decode.hip): rebuild (__graft_entry__.build())" % name)
        fn = getattr(L, name)
        fn.restype, fn.argtypes = res, args
    _bound = True
    return L


def _library():
    L = lib.load()
    if not _bound:
        _bind(L)
    return staging.checked_library("tiff", (("maf_tiff_struct_sizes", 3),), [HEADER_DT.itemsize, IMAGE_DT.itemsize, STRIP_DT.itemsize], "maf_tiff_* structs")


status_text = partial(staging.status_text, _STATUS_TEXT)


def decode(files, device=None, stream=None, check=True, taps=None, ignore_orientation=False):
    """Decode a list of TIFF files (bytes-like objects or paths; mixed sizes, compressions, bit depths and byte orders welcome) on the device
    -> a list of uint8 [h_i, w_i, 3] BGR CUDA tensors (views of one allocation), libtiff's pixels as Pillow returns them; they go into
    letterbox / eval_batch / detect_frames / train_batch as they are.  With check=True (the default) the per-image status words are read
    once after the launches (the call's one synchronisation) and a fault raises MafError naming the file and its status bits; check=False
    returns (frames, status int32 [B]) without synchronising.  `stream`: a torch.cuda.Stream to work on (default: the current one).
    `ignore_orientation`: take a file whose Orientation is not 1 and return its stored pixels.  `taps`: a dict that receives the
    intermediate buffers (the decompressed rows, the image and strip tables) — tests and the probe."""
    tables = {}

    def build(datas, infos):
        hdr, images, strips, palette = build_blob(infos)
        tables["strips"] = strips
        return hdr, images, lambda host: fill_blob(host, hdr, images, strips, palette, datas, infos)

    def launch(L, s, blob, hdr, out, status):
        import torch
        rows = torch.empty(int(hdr["rows_bytes"]), dtype=torch.uint8, device=s.dev)
        lib.check(L.maf_tiff_decode(s.host.ctypes.data, blob.data_ptr(), rows.data_ptr(), out.data_ptr(), status.data_ptr(), s.stream.cuda_stream))
        return dict(rows=rows, strips=tables["strips"])

    return staging.decode_files("tiff.decode", files, partial(parse, ignore_orientation=ignore_orientation), build, _library, launch, _STATUS_TEXT, True,
                                device, stream, check, taps)
