"""File bytes in, frames out, whatever the kind: the router in front of jpeg.py, png.py and (opt-in) webp.py.

A folder of the reference's loaders (IMG_FORMATS of yolov6/data/datasets.py, LoadData of yolov6/core/inferer.py) mixes JPEG and PNG files;
decode(files) sniffs each file's signature, hands the JPEG files to jpeg.decode and the PNG files to png.decode (one call each, so each kind
keeps its one host -> device copy and its one chain of launches) and returns the frames in input order.  With webp=True the RIFF / WEBP files
of the list go to webp.decode in one call of their own (lossless files; webp.py names what it refuses); without the flag nothing changes.
With webp=True and lossy=True the files among them whose image chunk is `VP8 ` (lossy) go to webp_lossy.decode instead, again in one call.
With tiff=True the files that begin `II*\\0` or `MM\\0*` go to tiff.decode in one call of their own (tiff.py names what it refuses).
With bmp=True the files that begin `BM` and name one of bmp.HEADER_SIZES at byte 14 go to bmp.decode in one call of their own (bmp.py names
what it refuses).  That covers the reference's IMG_FORMATS: an mpo file is a JPEG followed by more JPEGs and goes to jpeg.decode, which
decodes its first frame (what cv2.imread returns); a dng file stays on the host (tiff.py refuses a file with a DNGVersion tag).

The other way: encode(frames, suffixes) is the router in front of jpeg_encode.py, png_encode.py, tiff_encode.py and bmp_encode.py.  The
reference's cv2.imwrite(save_path, img_src) picks its encoder by the extension save_path keeps from the source file; so does encode, one call
per format present.  With webp_lossless=True (or a dict of webp_encode.encode's keyword arguments) the .webp files of the call go to
webp_encode.encode in one call of their own (lossless VP8L, what cv2.imwrite writes without parameters; webp_encode.py names what it does not
claim); with webp_lossy=True (or a dict of webp_lossy_encode.encode's keyword arguments: quality, base_q, filter_level, ...) they go to
webp_lossy_encode.encode instead (lossy VP8, what cv2.imwrite writes with IMWRITE_WEBP_QUALITY); giving both is an error; without either .webp
is refused as before.
"""
from . import bmp as bmp_codec, bmp_encode, jpeg, jpeg_encode, png, png_encode, staging, tiff as tiff_codec, tiff_encode, webp as webp_codec, webp_encode, webp_lossy, webp_lossy_encode
from .lib import MafError

ENCODERS = {"jpeg": jpeg_encode.encode, "png": png_encode.encode, "tiff": tiff_encode.encode, "bmp": bmp_encode.encode}
SUFFIX_FORMAT = {".jpg": "jpeg", ".jpeg": "jpeg", ".mpo": "jpeg", ".png": "png", ".tif": "tiff", ".tiff": "tiff", ".bmp": "bmp"}


def _lossy(data):
    """True where the first image chunk of a RIFF / WEBP file is `VP8 ` (a container webp.riff_chunks refuses is left to webp.decode to name)."""
    try:
        for cc, _, _, _ in webp_codec.riff_chunks(data):
            if cc in (b"VP8 ", b"VP8L"):
                return cc == b"VP8 "
    except MafError:
        pass
    return False


def kind(data, webp=False, lossy=False, tiff=False, bmp=False):
    """'jpeg' or 'png' by the signature of a file's bytes, with webp=True also 'webp' (RIFF....WEBP) and, with lossy=True as well,
    'webp_lossy' for such a file with a `VP8 ` image chunk, with tiff=True also 'tiff' (II*\\0 or MM\\0*), with bmp=True also 'bmp' (BM and a DIB
    header size bmp.py knows at byte 14), else None."""
    if bmp and data[:2] == b"BM" and len(data) >= 18 and int.from_bytes(data[14:18], "little") in bmp_codec.HEADER_SIZES:
        return "bmp"
    if tiff and data[:4] in (b"II*\0", b"MM\0*"):
        return "tiff"
    if webp and data[:4] == b"RIFF" and data[8:12] == b"WEBP":
        return "webp_lossy" if lossy and _lossy(data) else "webp"
    if data[:8] == png.SIGNATURE:
        return "png"
    if data[:2] == b"\xff\xd8":
        return "jpeg"
    return None


def decode(files, device=None, stream=None, check=True, progressive=False, ignore_orientation=False, interlaced=False, apply_orientation=False, webp=False,
           lossy=False, tiff=False, bmp=False):
    """Decode a list of JPEG and PNG files (bytes-like objects or paths, in any mix) on the device -> a list of uint8 [h_i, w_i, 3] BGR CUDA
    tensors in input order, what cv2.imread returns for each file.  `progressive`, `ignore_orientation` and `apply_orientation` go to jpeg.decode, `interlaced` to
    png.decode (the last two only when set).  webp=True also takes lossless WebP files (webp.decode, which is handed `ignore_orientation` too),
    webp=True with lossy=True lossy ones as well (webp_lossy.decode, handed the same), tiff=True TIFF files (tiff.decode, handed the same),
    bmp=True BMP files (bmp.decode).  With
    check=False -> (frames, status int32 [len(files)] on the device: each file's status word of its own decoder, merged on `stream` behind the
    decoders' launches) without synchronising."""
    files = list(files)
    if not files:
        raise MafError("frames.decode: no files")
    datas, groups = [], {"jpeg": [], "png": [], "webp": [], "webp_lossy": [], "tiff": [], "bmp": []}
    for i, f in enumerate(files):
        d = staging.file_bytes(f)
        k = "bmp" if bmp and kind(d, bmp=True) == "bmp" else "tiff" if tiff and kind(d, tiff=True) == "tiff" else kind(d, webp, lossy) if lossy else kind(d, webp)
        if k is None:
            raise MafError("%s: neither a JPEG nor a PNG signature" % staging.file_name(f, i))
        datas.append(d)
        groups[k].append(i)
    frames, words, order = [None] * len(files), [], []
    for k, idx in groups.items():
        if not idx:
            continue
        sub = [datas[i] for i in idx]
        try:
            if k == "jpeg":
                got = jpeg.decode(sub, device=device, stream=stream, ignore_orientation=ignore_orientation, check=check, progressive=progressive,
                                  **(dict(apply_orientation=True) if apply_orientation else {}))
            elif k == "png":
                got = png.decode(sub, device=device, stream=stream, check=check, **(dict(interlaced=True) if interlaced else {}))
            elif k == "webp":
                got = webp_codec.decode(sub, device=device, stream=stream, check=check, ignore_orientation=ignore_orientation)
            elif k == "tiff":
                got = tiff_codec.decode(sub, device=device, stream=stream, check=check, ignore_orientation=ignore_orientation)
            elif k == "bmp":
                got = bmp_codec.decode(sub, device=device, stream=stream, check=check)
            else:
                got = webp_lossy.decode(sub, device=device, stream=stream, check=check, ignore_orientation=ignore_orientation)
        except MafError as e:
            # the decoders number the files of their own call: say which input each one is
            raise type(e)("%s [%s files of this call are inputs %s]" % (e, k, idx)) from None
        if not check:
            got, st = got
            words.append(st)
            order += idx
        for i, fr in zip(idx, got):
            frames[i] = fr
    if check:
        return frames
    # The status words were written on `stream` (default: the current one) by the decoders' launches, so they are merged THERE, behind those
    # launches: the words of the decoders' calls back to back, then brought into input order by an index that travels in a pinned buffer
    # (non_blocking: the host does not wait for it either).
    import torch
    dev = words[0].device
    st = stream if stream is not None else torch.cuda.current_stream(dev)
    inverse = [0] * len(files)
    for at, i in enumerate(order):
        inverse[i] = at
    with torch.cuda.device(dev), torch.cuda.stream(st):
        index = torch.tensor(inverse, dtype=torch.int64).pin_memory().to(dev, non_blocking=True)
        status = torch.cat(words).index_select(0, index)
    return frames, status


def encode(frames, suffixes, rects=None, webp_lossless=None, webp_lossy=None, **per_format):
    """Encode frames (a list of uint8 [h, w, 3] BGR CUDA tensors, or one [B, h, w, 3] tensor) to files on the device, each in the format its
    suffix names -> list[bytes] in input order.  `suffixes`: one per output file (per frame, or per rectangle where `rects`, a host int array
    [R, 5] of (frame index, x1, y1, x2, y2), is given), taken case-insensitively as cv2.imwrite takes save_path's: .jpg / .jpeg / .mpo go to
    jpeg_encode.encode, .png to png_encode.encode, .tif / .tiff to tiff_encode.encode, .bmp to bmp_encode.encode, in one call per format
    present.  `per_format`: jpeg=, png=, tiff=, bmp=, each a dict of keyword arguments for that encoder (quality, filter, rows_per_strip,
    stream, ...).  `webp_lossless`: None refuses .webp; True, or a dict of keyword arguments for webp_encode.encode (predictor_bits, stream),
    sends the .webp files to it, in one call, in input order with the rest.  `webp_lossy`: likewise for webp_lossy_encode.encode (quality,
    base_q, filter_level, log2_parts, stream); webp_lossless and webp_lossy together are an error.  Reading the files back is where this synchronises, once per
    format.  Any other suffix (.webp without webp_lossless, .dng, ...) raises."""
    import numpy as np
    import torch
    if not torch.is_tensor(frames):                          # a [B, h, w, 3] tensor is indexed like the list; the encoders make every check of the frames
        frames = list(frames)
    unknown = sorted(set(per_format) - set(ENCODERS))
    if unknown:
        raise MafError("frames.encode: per-format arguments are jpeg=, png=, tiff= and bmp=, got %s" % ", ".join(unknown))
    if webp_lossless is not None and webp_lossless is not True and not isinstance(webp_lossless, dict):
        raise MafError("frames.encode: webp_lossless is None, True or a dict of keyword arguments for webp_encode.encode, got %r" % (webp_lossless,))
    encoders, suffix_format = ENCODERS, SUFFIX_FORMAT
    if webp_lossless is not None:
        encoders, suffix_format = dict(ENCODERS, webp=webp_encode.encode), dict(SUFFIX_FORMAT, **{".webp": "webp"})
        per_format = dict(per_format, webp=webp_lossless if isinstance(webp_lossless, dict) else {})
    if webp_lossy is not None:
        if webp_lossy is not True and not isinstance(webp_lossy, dict):
            raise MafError("frames.encode: webp_lossy is None, True or a dict of keyword arguments for webp_lossy_encode.encode, got %r" % (webp_lossy,))
        if webp_lossless is not None:
            raise MafError("frames.encode: webp_lossless and webp_lossy are both given: a .webp file is written one way")
        encoders, suffix_format = dict(ENCODERS, webp=webp_lossy_encode.encode), dict(SUFFIX_FORMAT, **{".webp": "webp"})
        per_format = dict(per_format, webp=webp_lossy if isinstance(webp_lossy, dict) else {})
    suffixes = [suffixes] if isinstance(suffixes, str) else list(suffixes)
    ra = None
    if rects is not None:
        ra = np.asarray(rects.cpu() if isinstance(rects, torch.Tensor) else rects)
    n = len(frames) if ra is None else len(ra)
    if len(suffixes) != n:
        raise MafError("frames.encode: %d suffixes for %d files (one per %s)" % (len(suffixes), n, "frame" if ra is None else "rectangle"))
    groups = {}
    for i, sfx in enumerate(suffixes):
        fmt = suffix_format.get(sfx.lower()) if isinstance(sfx, str) else None
        if fmt is None:
            raise MafError("frames.encode: file %d has suffix %r: no device encoder exists for it (there is one for %s)" % (i, sfx, ", ".join(suffix_format)))
        groups.setdefault(fmt, []).append(i)
    batches = []
    for fmt, idx in groups.items():                          # every format's launches are queued before any file is read back
        kw = dict(per_format.get(fmt) or {})
        try:
            if ra is None:
                batches.append((idx, encoders[fmt]([frames[i] for i in idx], **kw)))
            else:
                batches.append((idx, encoders[fmt](frames, rects=ra[idx], **kw)))     # all frames: a rectangle names its frame by the caller's index
        except MafError as e:
            # the encoders number the files of their own call: say which input each one is
            raise type(e)("%s [%s files of this call are inputs %s]" % (e, fmt, idx)) from None
    files = [None] * n
    for idx, enc in batches:
        for i, data in zip(idx, enc.files()):
            files[i] = data
    return files
